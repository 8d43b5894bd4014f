#!/usr/bin/env python3
"""Diagnostic: where a step of the persistent ConditionedNCA grow (csrc/nca_cond_persist.hip) spends its time, from the stamps build
(`make stamps`: -DNCA_STAMPS).  Every workgroup sums device wall-clock time per phase over the steps; printed as us per step
(median and max over workgroups):  poll = waiting for / loading the neighbours' band, life = life mask + resolved alpha,
stage = pre-life mask + fire mask + z tile, mlp = perception + UpdateNet + residual, publish = state -> LDS / history + band pairs
out.  `python tools/stamp_persist.py [B C HW T]` (default 8 20 64 64)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-stylization-with-nca_amd")
os.environ.setdefault("NCAHIP_LIB", os.path.join(PKG, "libncahip_stamps.so"))
sys.path[:0] = [ROOT, PKG]
import torch

from ncahip import ops

B, C, HW, T = (int(v) for v in (sys.argv[1:5] if len(sys.argv) >= 5 else (8, 20, 64, 64)))
L = ops.lib()
L.nca_debug_set_stamp_buffer_persist.argtypes = [ctypes.c_void_p]
gen = torch.Generator().manual_seed(0)
mk = lambda *s, k=1.0: (torch.randn(*s, generator=gen) * k)
w = ops.CondWeights(mk(3 * C, 1, 3, 3, k=0.3), mk(64, 3 * C, 1, 1, k=(3 * C) ** -0.5), mk(64, k=0.1), mk(64, 64, 1, 1, k=0.125),
                    mk(64, k=0.1), mk(C, 64, 1, 1, k=0.005), torch.zeros(1, device="cuda"))
x = torch.rand(B, C, HW, HW, generator=gen).cuda()
goal = (torch.randn(B, C - 4, HW, HW, generator=gen) * 0.5).cuda()
tiles = B * (HW // 16) ** 2
buf = torch.zeros(tiles * 8, dtype=torch.int64, device="cuda")
names = ["poll", "life", "stage", "mlp", "publish", "finalize"]
for hist in (True, False):
    ops.cond_grow(x, T, goal, None, w, 3, seed=1, keep_history=hist)          # warm-up
    L.nca_debug_set_stamp_buffer_persist(buf.data_ptr())
    ops.cond_grow(x, T, goal, None, w, 3, seed=1, keep_history=hist)
    torch.cuda.synchronize()
    L.nca_debug_set_stamp_buffer_persist(None)
    v = buf.view(tiles, 8)[:, :6].double().cpu() / 100.0     # wall clock: 100 MHz -> us
    med, mx = v.median(dim=0).values, v.max(dim=0).values
    print(json.dumps({"B": B, "C": C, "HW": HW, "T": T, "history": hist,
                      "us_per_step_median": {n: round(float(med[i]) / (T if n != "finalize" else 1), 3) for i, n in enumerate(names)},
                      "us_per_step_max": {n: round(float(mx[i]) / (T if n != "finalize" else 1), 3) for i, n in enumerate(names)}}))
