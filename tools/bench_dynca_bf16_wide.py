#!/usr/bin/env python3
"""fp32 against the wide range of the opt-in bf16-MFMA DyNCA step (ops.dynca_precision('bf16_wide'): C <= 32, fc <= 256), one JSON
line per case, printed and appended to profiles/dynca_bf16_wide.jsonl (or the file given with --out).

Every case runs three arms ALTERNATING in one process -- f32, the mode, f32 again -- each timed with device events, median of 10
after 3 warm-ups; the two f32 arms put the run-to-run spread on record next to the difference that is being measured.  Cases:
  per_step  the per-step kernels, T = 8 steps per call: 4 x 32 x 512^2 with fc = 256 and conditioning (BASELINE configs[4]'s shape),
            8 x 20 x 256^2 with fc = 160, 8 x 16 x 256^2 with fc = 256; and 8 x 16 x 256^2 with fc = 128 under 'bf16' (a narrow shape:
            the path that existed before the wide range)
  clip      ncahip.video.stylize_clip, 64 frames at 256^2, step_n = 8, a C = 20 / fc = 160 edge-conditioned model, f32 / bf16_wide
--lib FILE times another build of the library (an older one, to show that the paths it has did not move): its rows carry
"library": FILE's name, the arms of the wide range are left out (the mode is set through ncahip_dynca_precision alone) and only the
fp32 arms and the (16, 128) 'bf16' row are run.
mfma_per_group: matrix instructions per group of 16 cells and step, from the kernels' loop structure.
usage: python tools/bench_dynca_bf16_wide.py [per_step] [clip] [--lib FILE] [--out FILE]"""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]
import torch

from ncahip import _capi, ops

DEV = "cuda"
OTHER_LIB = None      # --lib: the name the rows carry


def set_mode(mode):
    """ops.set_dynca_precision; another build of the library may lack the range export, and takes 'f32' / 'bf16' at C level"""
    if OTHER_LIB is None:
        ops.set_dynca_precision(mode)
    else:
        assert mode in ("f32", "bf16"), mode
        assert ops.lib().ncahip_dynca_precision(("f32", "bf16").index(mode)) in (0, 1)


def mfma_per_group(C, fc, cc):
    """fp32: one launch per 128-wide slice, each with its own layer-1 chain; the mode: one launch, eight k values per instruction"""
    cp = 12 if C <= 12 and fc <= 96 else 16 if C <= 16 else 32
    k1s, m2t = cp + (1 if cc else 0), (cp + 15) // 16
    f32 = sum((min(128, fc - h0) + 15) // 16 * (k1s + 4 * m2t) for h0 in range(0, fc, 128)) if fc > 128 else (
        (96 if cp == 12 else 128) // 16 * (k1s + 4 * m2t))
    fcp = 96 if cp == 12 else 128 if fc <= 128 else 256
    return {"f32": f32, "bf16": fcp // 16 * ((k1s + 7) // 8) + fcp // 32 * m2t}


def timed_arms(fn, arms, iters=10, warm=3):
    """fn() under each arm's precision, the arms alternating within every iteration; {arm: (median ms, min ms)}"""
    def run(mode):
        set_mode(mode)
        try:
            fn(mode)
        finally:
            set_mode("f32")
    for _ in range(warm):
        for _, mode in arms:
            run(mode)
    torch.cuda.synchronize()
    res = {name: [] for name, _ in arms}
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(arms) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(arms):
            run(mode)
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(arms):
            res[name].append(ev[i].elapsed_time(ev[i + 1]))
    ops.check_errors()
    return {name: (statistics.median(v), min(v)) for name, v in res.items()}


def arms_of(mode):
    if OTHER_LIB is not None and mode == "bf16_wide":
        return (("f32", "f32"), ("f32_again", "f32"))
    return (("f32", "f32"), (mode, mode), ("f32_again", "f32"))


def weights(C, fc, cc, gen):
    k1 = 4 * C + cc
    return ops.DyncaWeights(torch.randn(fc, k1, generator=gen) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=gen) * 0.1,
                            torch.randn(C, fc, generator=gen) * (0.02 / fc ** 0.5), torch.zeros(C), torch.zeros(1, device=DEV))


def steps_case(out, path, mode, B, C, fc, cc, H, W, T):
    gen = torch.Generator().manual_seed(0)
    w = weights(C, fc, cc, gen)
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    cond = (torch.rand(B, cc, H, W, generator=gen) * 2 - 1).to(DEV) if cc else None
    arms = arms_of(mode)
    ops.persistent_steps = False
    try:
        last = {}

        def fn(m):
            last[m] = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1)[0]
        res = timed_arms(fn, arms)
    finally:
        ops.persistent_steps = True
    us = {name: {"us_per_step": a / T * 1e3, "min_us_per_step": b / T * 1e3} for name, (a, b) in res.items()}
    extra = {}
    if mode in res:
        extra = {"mode_over_f32": res[mode][0] / res["f32"][0], "mode_changes_the_result": not torch.equal(last[mode], last["f32"])}
    out(path=path, mode=mode, B=B, C=C, fc=fc, c_cond=cc, HW=[H, W], steps_per_call=T, **us, **extra,
        f32_again_over_f32=res["f32_again"][0] / res["f32"][0], mfma_per_group=mfma_per_group(C, fc, cc))


def clip_case(out, C, fc):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    n_frames, step_n, S = 64, 8, 256
    torch.manual_seed(0)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0], device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
    arms = arms_of("bf16_wide")
    routes, runs = set(), {name: [] for name, _ in arms}
    for it in range(13):                      # 3 warm-ups + 10, the arms alternating
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(arms) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(arms):
            video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8, precision=mode)
            routes.add(video.stylize_clip.last_path)
            ev[i + 1].record()
        torch.cuda.synchronize()
        if it >= 3:
            for i, (name, _) in enumerate(arms):
                runs[name].append(ev[i].elapsed_time(ev[i + 1]))
    ops.check_errors()
    res = {name: {"us_per_frame": statistics.median(v) / n_frames * 1e3, "min_us_per_frame": min(v) / n_frames * 1e3} for name, v in runs.items()}
    extra = {"mode_over_f32": res["bf16_wide"]["us_per_frame"] / res["f32"]["us_per_frame"]} if "bf16_wide" in res else {}
    out(path="stylize_clip", mode="bf16_wide", C=C, fc=fc, HW=[S, S], frames=n_frames, step_n=step_n, masks="philox", io="uint8", route=sorted(routes),
        **res, **extra, f32_again_over_f32=res["f32_again"]["us_per_frame"] / res["f32"]["us_per_frame"], mfma_per_group=mfma_per_group(C, fc, 3))


def main(argv):
    global OTHER_LIB
    dest = os.path.join(ROOT, "profiles", "dynca_bf16_wide.jsonl")
    if "--out" in argv:
        i = argv.index("--out")
        dest = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if "--lib" in argv:
        i = argv.index("--lib")
        _capi.LIB_PATH = os.path.abspath(argv[i + 1])
        OTHER_LIB = os.path.basename(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
        probe = ctypes.CDLL(_capi.LIB_PATH)                        # an older library lacks the newer exports: bind what it has
        for name in [n for n in _capi.SIGNATURES if not hasattr(probe, n)]:
            del _capi.SIGNATURES[name]
    legs = argv or ["per_step", "clip"]
    ops.selftest()

    def out(**kw):
        if OTHER_LIB is not None:
            kw = dict(library=OTHER_LIB, **kw)
        line = json.dumps(kw)
        print(line, flush=True)
        with open(dest, "a") as f:
            f.write(line + "\n")

    if "per_step" in legs:
        steps_case(out, "per_step_configs4", "bf16_wide", 4, 32, 256, 3, 512, 512, 8)
        steps_case(out, "per_step_c20", "bf16_wide", 8, 20, 160, 3, 256, 256, 8)
        steps_case(out, "per_step_fc256", "bf16_wide", 8, 16, 256, 3, 256, 256, 8)
        steps_case(out, "per_step_batch_narrow", "bf16", 8, 16, 128, 3, 256, 256, 8)
    if "clip" in legs and OTHER_LIB is None:
        clip_case(out, 20, 160)


if __name__ == "__main__":
    main(sys.argv[1:])
