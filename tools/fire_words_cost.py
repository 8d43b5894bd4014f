#!/usr/bin/env python3
"""What one fire-word launch costs a ConditionedNCA grow and what it saves per step ("Fire words"): the
break-even behind fire_words_pay in csrc/nca_capi.hip.

At bench.py's shape (8 x 16 x 256^2, or the shape given as B C H W) the same grow of T steps runs with its masks drawn beforehand
(ncahip_debug_force_generic bits 16-23 = 255: one chunk, and the length / grid rule this tool measures is waived) and drawn in the
kernel (bit 7), alternating, for a ladder of T; device events around each call, median of REPS.  d(T) = on - off is the launch's
cost minus T times the per-step saving; a least-squares line through the d(T) of the grows that drew beforehand (`launches` = 1)
gives both, and break-even = cost / saving.  One JSON line per T, then the fit.
usage: python tools/fire_words_cost.py [B C H W] > profiles/<tag>_fire_words_cost.jsonl"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import bench  # noqa: E402
from ncahip import ops  # noqa: E402

REPS, ON, OFF = 40, 255 << 16, 128
LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 32, 64)


def main():
    B, C, H, W = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (bench.B, bench.C, bench.H, bench.W)
    assert C == bench.C, "bench.make_weights is written for C = %d" % bench.C
    dev = torch.device("cuda", 0)
    ops.selftest(dev)
    prm = bench.make_weights(torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1234)
    xd = torch.rand(B, C, H, W, generator=g).to(dev)
    gd = (torch.randn(B, bench.GOAL_CH, H, W, generator=g) * 0.5).to(dev)
    w = ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                        prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], xd)
    states = torch.empty(2, B, C, H, W, device=dev)
    pre = torch.empty(2, B, H, W, device=dev, dtype=torch.uint8)
    out = torch.empty_like(xd)
    L, st = ops.lib(), torch.cuda.current_stream().cuda_stream

    def grow(T, bits):
        ops.force_generic(bits)
        states[0].copy_(xd)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.check(L.ncahip_cond_grow_fwd_f32(states.data_ptr(), pre.data_ptr(), 2, T, out.data_ptr(), gd.data_ptr(), bench.GOAL_CH, None,
                                             w.wp.data_ptr(), w.w1.data_ptr(), w.b1.data_ptr(), w.w2.data_ptr(), w.b2.data_ptr(),
                                             w.w3.data_ptr(), B, C, H, W, bench.HIDDEN, bench.ALIVE_CH, 0.1, 0.5, -10.0, 10.0, 42, 0, st),
                  "cond_grow")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3, L.ncahip_debug_fire_word_launches()

    # the fire-word launch alone, back to back (device events around 20 launches)
    words = torch.empty(64 * B * (H // 4) * (W // 16), device=dev, dtype=torch.int64)
    for Tc in (1, 8, 64):
        us = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                ops.check(L.ncahip_cond_fire_words(words.data_ptr(), Tc, B, H, W, 0.5, 42, 0, st), "fire words")
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / 20)
        print(json.dumps({"leg": "fire_words_alone", "shape": [B, C, H, W], "Tc": Tc, "us_per_launch_back_to_back": round(statistics.median(us), 3)}))

    xs, ys = [], []
    try:
        for T in LADDER:
            for _ in range(3):
                grow(T, ON), grow(T, OFF)
            on, off, n_on = [], [], 0
            for _ in range(REPS):
                t, n_on = grow(T, ON)
                on.append(t)
                off.append(grow(T, OFF)[0])
            m_on, m_off = statistics.median(on), statistics.median(off)
            print(json.dumps({"leg": "grow", "shape": [B, C, H, W], "T": T, "launches": n_on, "on_us": round(m_on, 2), "off_us": round(m_off, 2),
                              "on_minus_off_us": round(m_on - m_off, 2)}), flush=True)
            if n_on:
                xs.append(float(T))
                ys.append(m_on - m_off)
    finally:
        ops.force_generic(0)
    if len(xs) >= 2:
        mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
        slope = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
        cost = my - slope * mx
        print(json.dumps({"leg": "fit", "launch_cost_us": round(cost, 2), "saving_us_per_step": round(-slope, 3),
                          "break_even_steps": round(cost / -slope, 2) if slope < 0 else None}))


if __name__ == "__main__":
    main()
