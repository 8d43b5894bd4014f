#!/usr/bin/env python3
"""fp32 against the opt-in bf16-MFMA TRAINING mode of DyNCA (models.dynca.DyNCA.train_precision, include/ncahip.h), one JSON line per
case, printed and appended to profiles/dynca_train_bf16.jsonl (or the file given with --out).

Every case runs three arms ALTERNATING in one process -- f32, bf16, f32 again -- each timed with device events, median of 10 after 3
warm-ups; the two f32 arms put the run-to-run spread on record next to the difference that is being measured.  Cases:
  bwd_step  the backward alone (ops.dynca_nsteps_backward over a kept history of T = 8, per step) at 8 x 16 x 256^2, fc = 128 and at
            4 x 12 x 256^2, fc = 96, c_cond = 3, single- and two-scale
  fwd_bwd   forward with history + backward of T = 32 at the same two shapes (single-scale)
  trainer   DyNCATrainer.step with a stand-in loss at the reference's defaults (batch 2, 256^2, C = 12, fc = 96, T in [32, 128) as drawn)
mfma_per_group: matrix instructions of the backward's MLP kernel per group of 16 cells and step, from its loop structure
(csrc/nca_dynca_step.h): f32 = layer 1 + dh + dL/dy + dW2 on 16x16x4_f32; bf16 = layer 1 and dL/dy on 16x16x32_bf16, dh on 16x16x16_bf16,
dW2 one 16x16x32_bf16 per hidden tile and PAIR of groups.
usage: python tools/bench_dynca_train_precision.py [bwd_step] [fwd_bwd] [trainer] [--out FILE]"""
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
    k1s, m1t, mj = cp + (1 if cc else 0), fcp // 16, cp // 4
    return {"f32": m1t * k1s + m1t * 4 + m1t * 4 * mj + m1t * 4,
            "bf16": m1t * ((k1s + 7) // 8) + m1t + (m1t // 2) * mj + m1t / 2}


def timed_arms(fn, iters=10, warm=3):
    """fn(mode) for each arm, the arms alternating within every iteration; {arm: (median ms, min ms)}"""
    for _ in range(warm):
        for _, mode in ARMS:
            fn(mode)
    torch.cuda.synchronize()
    res = {name: [] for name, _ in ARMS}
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(ARMS) + 1)]
        ev[0].record()
        for i, (_, mode) in enumerate(ARMS):
            fn(mode)
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i, (name, _) in enumerate(ARMS):
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


def ratios(res):
    return dict(bf16_over_f32=res["bf16"][0] / res["f32"][0], f32_again_over_f32=res["f32_again"][0] / res["f32"][0])


def bwd_step_case(out, B, C, fc, cc, H, W, two, T=8):
    w, x, cond, g = inputs(B, C, fc, cc, H, W)
    hist = {}
    for mode in ("f32", "bf16"):                       # each backward reads the history of its own forward
        with ops.dynca_precision(mode):
            hist[mode] = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, keep_history=True, two_scale=two)[1].clone()
    res = timed_arms(lambda mode: ops.dynca_nsteps_backward(hist[mode], cond, None, w, g, None, T, "circular", 0.5, 1, 0, two_scale=two,
                                                            precision=mode))
    us = {name: {"us_per_step": a / T * 1e3, "min_us_per_step": b / T * 1e3} for name, (a, b) in res.items()}
    out(case="bwd_step", B=B, C=C, fc=fc, c_cond=cc, two_scale=two, HW=[H, W], steps_per_call=T, **us, **ratios(res),
        mfma_per_group=mfma_per_group(C, fc, cc))


def fwd_bwd_case(out, B, C, fc, cc, H, W, T=32):
    w, x, cond, g = inputs(B, C, fc, cc, H, W)

    def run(mode):
        with ops.dynca_precision(mode):
            states = ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, keep_history=True)[1]
        ops.dynca_nsteps_backward(states, cond, None, w, g, None, T, "circular", 0.5, 1, 0, precision=mode)
    res = timed_arms(run)
    ms = {name: {"ms_per_call": a, "min_ms_per_call": b, "us_per_step": a / T * 1e3} for name, (a, b) in res.items()}
    out(case="fwd_bwd", B=B, C=C, fc=fc, c_cond=cc, two_scale=False, HW=[H, W], steps_per_call=T, **ms, **ratios(res))


def trainer_case(out):
    from ncahip.dynca_trainer import DyNCATrainer
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="replicate", conditioning="pos_emb", device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    target = torch.linspace(-0.5, 0.5, 3, device=DEV).view(1, 3, 1, 1)
    tr = DyNCATrainer(m, lambda d: ((d["generated_image_list"][0] - target) ** 2).mean(), pool_size=16, size=(256, 256), batch_size=2,
                      nca_steps=(32, 128), device=torch.device(DEV))
    steps = []

    def run(mode):
        m.train_precision = mode
        tr.iteration = 1                               # the same drawn T and slots in every arm and iteration (the reseed is per iteration)
        steps.append(tr.step()[1])
    res = timed_arms(run)
    assert len(set(steps)) == 1, steps
    ms = {name: {"ms_per_iteration": a, "min_ms_per_iteration": b} for name, (a, b) in res.items()}
    out(case="trainer_step", B=2, C=12, fc=96, c_cond=2, HW=[256, 256], T=steps[0], loss="stand-in (mean squared distance of the image to a constant)",
        **ms, **ratios(res))


def main(argv):
    dest = os.path.join(ROOT, "profiles", "dynca_train_bf16.jsonl")
    if "--out" in argv:
        i = argv.index("--out")
        dest = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    legs = argv or ["bwd_step", "fwd_bwd", "trainer"]
    ops.selftest()

    def out(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        with open(dest, "a") as f:
            f.write(line + "\n")

    shapes = ((8, 16, 128, 3, 256, 256), (4, 12, 96, 3, 256, 256))
    if "bwd_step" in legs:
        for s in shapes:
            for two in (False, True):
                bwd_step_case(out, *s, two)
    if "fwd_bwd" in legs:
        for s in shapes:
            fwd_bwd_case(out, *s)
    if "trainer" in legs:
        trainer_case(out)


if __name__ == "__main__":
    main(sys.argv[1:])
