#!/usr/bin/env python3
"""fp32 against the opt-in bf16-MFMA DyNCA step (ops.dynca_precision), one JSON line per case, printed and appended to
profiles/dynca_bf16.jsonl (or the file given with --out).

Every case runs three arms ALTERNATING in one process -- f32, bf16, f32 again -- each timed with device events, median of 10 after 3
warm-ups; the two f32 arms put the run-to-run spread on record next to the difference that is being measured.  Cases:
  persist   B = 1, 256^2, T = 32 steps per call through the one-launch kernels (tools/bench_paths.py's video_B1 shapes)
  per_step  the per-step kernel at 8 x 16 x 256^2, fc = 128, and at 1 x 16 x 512^2 (one launch per step)
  clip      ncahip.video.stylize_clip, 64 frames at 256^2, step_n = 8, both shipped model shapes (two-scale), precision f32 / bf16
mfma_per_group: matrix instructions per group of 16 cells and step, from the kernels' loop structure.
usage: python tools/bench_dynca_precision.py [persist] [per_step] [clip] [--out FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]
import torch

from ncahip import ops

DEV = "cuda"
ARMS = (("f32", "f32"), ("bf16", "bf16"), ("f32_again", "f32"))


def mfma_per_group(C, fc, cc):
    cp, fcp = (12, 96) if C <= 12 and fc <= 96 else (16, 128)
    k1s = cp + (1 if cc else 0)
    return {"f32": fcp // 16 * k1s + fcp // 4, "bf16": fcp // 16 * ((k1s + 7) // 8) + fcp // 32}


def timed_arms(fn, iters=10, warm=3):
    """fn() under each arm's precision, the arms alternating within every iteration; {arm: (median ms, min ms)}"""
    def run(mode):
        with ops.dynca_precision(mode):
            fn()
    for _ in range(warm):
        for _, mode in ARMS:
            run(mode)
    torch.cuda.synchronize()
    res = {name: [] for name, _ in ARMS}
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(ARMS) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(ARMS):
            run(mode)
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(ARMS):
            res[name].append(ev[i].elapsed_time(ev[i + 1]))
    ops.check_errors()
    return {name: (statistics.median(v), min(v)) for name, v in res.items()}


def weights(C, fc, cc, gen):
    k1 = 4 * C + cc
    return ops.DyncaWeights(torch.randn(fc, k1, generator=gen) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=gen) * 0.1,
                            torch.randn(C, fc, generator=gen) * (0.02 / fc ** 0.5), torch.zeros(C), torch.zeros(1, device=DEV))


def steps_case(out, path, B, C, fc, cc, H, W, T, two, persistent):
    gen = torch.Generator().manual_seed(0)
    w = weights(C, fc, cc, gen)
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    cond = (torch.rand(B, cc, H, W, generator=gen) * 2 - 1).to(DEV)
    ops.persistent_steps = persistent
    try:
        _, states = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, two_scale=two)
        assert (states is None) == persistent, "the case did not take the kernel it is meant to time"
        res = timed_arms(lambda: ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, two_scale=two))
    finally:
        ops.persistent_steps = True
    us = {name: {"us_per_step": a / T * 1e3, "min_us_per_step": b / T * 1e3} for name, (a, b) in res.items()}
    out(path=path, B=B, C=C, fc=fc, c_cond=cc, two_scale=two, HW=[H, W], steps_per_call=T, **us,
        bf16_over_f32=res["bf16"][0] / res["f32"][0], f32_again_over_f32=res["f32_again"][0] / res["f32"][0],
        mfma_per_group=mfma_per_group(C, fc, cc))


def clip_case(out, C, fc):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    n_frames, step_n, S = 64, 8, 256
    torch.manual_seed(0)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0, 1],
              device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
    res, routes = {}, set()
    runs = {name: [] for name, _ in ARMS}
    for it in range(13):                      # 3 warm-ups + 10, the arms alternating
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(ARMS) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(ARMS):
            video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8, precision=mode)
            routes.add(video.stylize_clip.last_path)
            ev[i + 1].record()
        torch.cuda.synchronize()
        if it >= 3:
            for i, (name, _) in enumerate(ARMS):
                runs[name].append(ev[i].elapsed_time(ev[i + 1]))
    ops.check_errors()
    res = {name: {"us_per_frame": statistics.median(v) / n_frames * 1e3, "min_us_per_frame": min(v) / n_frames * 1e3} for name, v in runs.items()}
    out(path="stylize_clip", C=C, fc=fc, two_scale=True, HW=[S, S], frames=n_frames, step_n=step_n, masks="philox", io="uint8",
        route=sorted(routes), **res, bf16_over_f32=res["bf16"]["us_per_frame"] / res["f32"]["us_per_frame"],
        f32_again_over_f32=res["f32_again"]["us_per_frame"] / res["f32"]["us_per_frame"], mfma_per_group=mfma_per_group(C, fc, 3))


def main(argv):
    dest = os.path.join(ROOT, "profiles", "dynca_bf16.jsonl")
    if "--out" in argv:
        i = argv.index("--out")
        dest = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    legs = argv or ["persist", "per_step", "clip"]
    ops.selftest()

    def out(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(dest, "a") as f:
            f.write(line + "\n")

    if "persist" in legs:
        for C, fc in ((12, 96), (16, 128)):
            for two in (False, True):
                steps_case(out, "video_B1_persistent", 1, C, fc, 2, 256, 256, 32, two, True)
    if "per_step" in legs:
        steps_case(out, "per_step_batch", 8, 16, 128, 3, 256, 256, 8, False, False)
        steps_case(out, "per_step_video_large", 1, 16, 128, 3, 512, 512, 8, False, False)
        steps_case(out, "per_step_video_B1", 1, 12, 96, 2, 256, 256, 32, False, False)
    if "clip" in legs:
        for C, fc in ((12, 96), (16, 128)):
            clip_case(out, C, fc)


if __name__ == "__main__":
    main(sys.argv[1:])
