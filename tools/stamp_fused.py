#!/usr/bin/env python3
"""Diagnostic: per-tile phase stamps of the fp32 producer/consumer step inside a grow at bench.py's shape, on the fused-steps launch
(default) and with one launch per step (ncahip_debug_force_generic bit 24) -- per role: the producer's period and its phases (the
wait for its tile buffer, the gate, the step view, the loads' issue, stage_tile, the pre mask drain), the consumer's tile time and
the time it waits for a staged tile.

Needs a library whose csrc/nca_cond_pc.hip was compiled with -DNCA_STAMPS=2 (never the shipped library), as
video-stylization-with-nca_amd/libncahip_stamps2.so or the path in NCAHIP_STAMPS_LIB.  The stamps of the grow's last step stay in
the buffer (a fused launch stamps every step's tiles anew).  s_memtime ticks (as tools/stamp_fire.py reports them), medians over all
waves of the role and the tiles 1..6 of each whose stamps are complete.  The stamps themselves cost time in every tile: compare the
two columns, not their absolute values.
usage: python tools/stamp_fused.py > profiles/<tag>_phases.txt"""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "video-stylization-with-nca_amd")
os.environ["NCAHIP_LIB"] = os.environ.get("NCAHIP_STAMPS_LIB", os.path.join(PKG, "libncahip_stamps2.so"))
sys.path[:0] = [ROOT, PKG]
import bench  # noqa: E402
from ncahip import ops  # noqa: E402

B, C, H, W, T = bench.B, bench.C, bench.H, bench.W, 16
dev = "cuda"
gen = torch.Generator().manual_seed(0)
prm = bench.make_weights(gen)
x = torch.rand(B, C, H, W, generator=gen).to(dev)
goal = (torch.randn(B, bench.GOAL_CH, H, W, generator=gen) * 0.5).to(dev)
w = ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                    prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], x)
L = ops.lib()
L.nca_debug_set_stamp_buffer_pc.argtypes = [ctypes.c_void_p]
ops.persistent_cond = False
NWG, TILES = 256, 8
buf = torch.zeros(NWG * 8 * TILES * 16 + NWG * 8 * 8, dtype=torch.int64, device=dev)


def med_diff(s, i, j, shift=0):
    """median of stamp j (of the tile `shift` later) - stamp i over the entries where both were written"""
    a = s[..., 1:7 - shift, i]
    b = s[..., 1 + shift:7, j]
    ok = (a > 0) & (b > 0)
    return float(np.median((b - a)[ok])) if ok.any() else float("nan")


def run(bits):
    ops.force_generic(bits)
    try:
        for _ in range(2):
            ops.cond_grow(x, T, goal, None, w, 3, seed=42)
        torch.cuda.synchronize()
        buf.zero_()
        L.nca_debug_set_stamp_buffer_pc(buf.data_ptr())
        ops.cond_grow(x, T, goal, None, w, 3, seed=42)
        torch.cuda.synchronize()
        L.nca_debug_set_stamp_buffer_pc(None)
        n = ops.fused_step_launches()
    finally:
        ops.force_generic(0)
    s = buf[:NWG * 8 * TILES * 16].cpu().numpy().reshape(NWG, 8, TILES, 16).astype(np.float64)
    cons, prod = s[:, 0:4], s[:, 4:8]
    return {"fused-steps launches of the grow": n,
            "producer period                        0 -> next 0": med_diff(prod, 0, 0, 1),
            "producer wait for its buffer, await(1)      0 -> 1": med_diff(prod, 0, 1),
            "producer gate                               1 -> 2": med_diff(prod, 1, 2),
            "producer step view                          2 -> 3": med_diff(prod, 2, 3),
            "producer loads' issue                       3 -> 8": med_diff(prod, 3, 8),
            "producer stage_tile                        8 -> 13": med_diff(prod, 8, 13),
            "producer pre mask drain                   13 -> 14": med_diff(prod, 13, 14),
            "producer hand-off, next tile's walk  14 -> next 0": med_diff(prod, 14, 0, 1),
            "producer busy (period less the wait)": med_diff(prod, 0, 0, 1) - med_diff(prod, 0, 1),
            "consumer period                        0 -> next 0": med_diff(cons, 0, 0, 1),
            "consumer wait for a staged tile, await(0)   0 -> 1": med_diff(cons, 0, 1),
            "consumer tile (staged -> stored)            1 -> 8": med_diff(cons, 1, 8),
            "consumer first group: perception            4 -> 5": med_diff(cons, 4, 5),
            "consumer first group: UpdateNet             5 -> 6": med_diff(cons, 5, 6),
            "consumer store_tile                         7 -> 8": med_diff(cons, 7, 8),
            "consumer hand-off, bookkeeping             8 -> 14": med_diff(cons, 8, 14)}


NO_FUSED = 1 << 24
a, b = run(0), run(NO_FUSED)
a2, b2 = run(0), run(NO_FUSED)
print("# tools/stamp_fused.py (%s): s_memtime ticks, medians; fused launch / one launch per step (bit 24), each measured twice"
      % os.path.basename(os.environ["NCAHIP_LIB"]))
print("%-56s %10s %10s %10s %10s" % ("", "fused", "per step", "fused (2)", "per step (2)"))
for k in a:
    print("%-56s %10.1f %10.1f %10.1f %10.1f" % (k, a[k], b[k], a2[k], b2[k]))
