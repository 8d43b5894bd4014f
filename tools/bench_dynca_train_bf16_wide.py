#!/usr/bin/env python3
"""fp32 against the WIDE range of the opt-in bf16-MFMA TRAINING mode of DyNCA (train_precision="bf16_wide": C <= 32, fc <= 256,
include/ncahip.h), one JSON line per case, printed and appended to profiles/dynca_train_bf16_wide.jsonl (or the file given with --out).

Every case runs three arms ALTERNATING in one process -- f32, the mode, f32 again -- each timed with device events, median of 10 after
3 warm-ups; the two f32 arms put the run-to-run spread on record next to the difference that is being measured.  Cases:
  bwd_step  the backward alone (ops.dynca_nsteps_backward over a kept history of T = 8, per step): 4 x 32 x 512^2 with fc = 256 and
            conditioning (BASELINE configs[4]'s shape), 8 x 20 x 256^2 with fc = 160, 8 x 16 x 256^2 with fc = 256; and 8 x 16 x 256^2 with
            fc = 128 under "bf16" (a narrow shape: the path that existed before the wide range)
  fwd_bwd   forward with history + backward of T = 32 at the last two wide shapes and the narrow one
  trainer   DyNCATrainer.step with a stand-in loss on a C = 32 / fc = 256 model (batch 2, 256^2, T in [32, 128) as drawn)
--lib FILE times another build of the library (an older one, to show that the paths it has did not move): its rows carry
"library": FILE's name, the arms of the wide range are left out and only the fp32 arms and the narrow "bf16" rows are run.
mfma_per_group: matrix instructions of the backward's MLP kernels per group of 16 cells and step, from their loop structure
(csrc/nca_dynca_step.h): f32 = per 128-wide slice layer 1 + dh + dL/dy + dW2 on 16x16x4_f32; the mode = per slice
layer 1 and dL/dy on 16x16x32_bf16, dh on 16x16x16_bf16 (one per channel tile), dW2 one 16x16x32_bf16 per channel tile, hidden tile and
PAIR of groups.
usage: python tools/bench_dynca_train_bf16_wide.py [bwd_step] [fwd_bwd] [trainer] [--lib FILE] [--out FILE]"""
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


def mfma_per_group(C, fc, cc):
    narrow = C <= 16 and fc <= 128
    cp = (12 if C <= 12 and fc <= 96 else 16) if narrow else (16 if C <= 16 else 32)
    k1s, mj, m2t = cp + (1 if cc else 0), cp // 4, (cp + 15) // 16
    f32 = bf = 0
    for h0 in range(0, fc, 128):
        m1t = (96 if cp == 12 else 128) // 16 if narrow else 8          # a slice is compiled at 128 hidden units
        f32 += m1t * k1s + m1t * 4 * m2t + m1t * 4 * mj + m1t * 4 * m2t
        bf += m1t * ((k1s + 7) // 8) + m1t * m2t + (m1t // 2) * mj + m1t * m2t / 2
    return {"f32": f32, "bf16": bf}


def arms_of(mode):
    if OTHER_LIB is not None and mode == "bf16_wide":
        return (("f32", "f32"), ("f32_again", "f32"))
    return (("f32", "f32"), (mode, mode), ("f32_again", "f32"))


def timed_arms(fn, arms, iters=10, warm=3):
    """fn(mode) for each arm, the arms alternating within every iteration; {arm: (median ms, min ms)}"""
    for _ in range(warm):
        for _, mode in arms:
            fn(mode)
    torch.cuda.synchronize()
    res = {name: [] for name, _ in arms}
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(arms) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(arms):
            fn(mode)
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(arms):
            res[name].append(ev[i].elapsed_time(ev[i + 1]))
    ops.check_errors()
    return {name: (statistics.median(v), min(v)) for name, v in res.items()}


def inputs(B, C, fc, cc, H, W):
    gen = torch.Generator().manual_seed(0)
    k1 = 4 * C + cc
    w = ops.DyncaWeights(torch.randn(fc, k1, generator=gen) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=gen) * 0.1,
                         torch.randn(C, fc, generator=gen) * (0.02 / fc ** 0.5), torch.zeros(C), torch.zeros(1, device=DEV))
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    cond = (torch.rand(B, cc, H, W, generator=gen) * 2 - 1).to(DEV)
    g = torch.randn(B, C, H, W, generator=gen).to(DEV)
    return w, x, cond, g


def ratios(res, mode):
    r = dict(f32_again_over_f32=res["f32_again"][0] / res["f32"][0])
    if mode in res:
        r["mode_over_f32"] = res[mode][0] / res["f32"][0]
    return r


def bwd_step_case(out, name, mode, B, C, fc, cc, H, W, T=8):
    w, x, cond, g = inputs(B, C, fc, cc, H, W)
    arms = arms_of(mode)
    hist = {}
    for m in {m for _, m in arms}:                     # each backward reads the history of its own forward
        with ops.dynca_precision(m):
            hist[m] = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, keep_history=True)[1].clone()
    res = timed_arms(lambda m: ops.dynca_nsteps_backward(hist[m], cond, None, w, g, None, T, "circular", 0.5, 1, 0, precision=m), arms)
    us = {n: {"us_per_step": a / T * 1e3, "min_us_per_step": b / T * 1e3} for n, (a, b) in res.items()}
    out(case="bwd_step", shape=name, mode=mode, B=B, C=C, fc=fc, c_cond=cc, HW=[H, W], steps_per_call=T, **us, **ratios(res, mode),
        mfma_per_group=mfma_per_group(C, fc, cc))


def fwd_bwd_case(out, name, mode, B, C, fc, cc, H, W, T=32):
    w, x, cond, g = inputs(B, C, fc, cc, H, W)

    def run(m):
        with ops.dynca_precision(m):
            states = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, keep_history=True)[1]
        ops.dynca_nsteps_backward(states, cond, None, w, g, None, T, "circular", 0.5, 1, 0, precision=m)
    res = timed_arms(run, arms_of(mode))
    ms = {n: {"ms_per_call": a, "min_ms_per_call": b, "us_per_step": a / T * 1e3} for n, (a, b) in res.items()}
    out(case="fwd_bwd", shape=name, mode=mode, B=B, C=C, fc=fc, c_cond=cc, HW=[H, W], steps_per_call=T, **ms, **ratios(res, mode))


def trainer_case(out):
    from ncahip.dynca_trainer import DyNCATrainer
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(32, 3, fc_dim=256, padding_mode="replicate", conditioning="pos_emb", device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    target = torch.linspace(-0.5, 0.5, 3, device=DEV).view(1, 3, 1, 1)
    tr = DyNCATrainer(m, lambda d: ((d["generated_image_list"][0] - target) ** 2).mean(), pool_size=16, size=(256, 256), batch_size=2,
                      nca_steps=(32, 128), device=torch.device(DEV))
    steps = []

    def run(mode):
        m.train_precision = mode
        tr.iteration = 1                               # the same drawn T and slots in every arm and iteration (the reseed is per iteration)
        steps.append(tr.step()[1])
    res = timed_arms(run, arms_of("bf16_wide"))
    assert len(set(steps)) == 1, steps
    ms = {n: {"ms_per_iteration": a, "min_ms_per_iteration": b} for n, (a, b) in res.items()}
    out(case="trainer_step", mode="bf16_wide", B=2, C=32, fc=256, c_cond=2, HW=[256, 256], T=steps[0],
        loss="stand-in (mean squared distance of the image to a constant)", **ms, **ratios(res, "bf16_wide"))


def main(argv):
    global OTHER_LIB
    dest = os.path.join(ROOT, "profiles", "dynca_train_bf16_wide.jsonl")
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
    legs = argv or ["bwd_step", "fwd_bwd", "trainer"]
    ops.selftest()

    def out(**kw):
        if OTHER_LIB is not None:
            kw = dict(library=OTHER_LIB, **kw)
        line = json.dumps(kw)
        print(line, flush=True)
        with open(dest, "a") as f:
            f.write(line + "\n")

    shapes = (("configs4", "bf16_wide", 4, 32, 256, 3, 512, 512), ("c20", "bf16_wide", 8, 20, 160, 3, 256, 256),
              ("fc256", "bf16_wide", 8, 16, 256, 3, 256, 256), ("batch_narrow", "bf16", 8, 16, 128, 3, 256, 256))
    if "bwd_step" in legs:
        for s in shapes:
            bwd_step_case(out, *s)
    if "fwd_bwd" in legs:
        for s in shapes[1:]:
            fwd_bwd_case(out, *s)
    if "trainer" in legs:
        trainer_case(out)


if __name__ == "__main__":
    main(sys.argv[1:])
