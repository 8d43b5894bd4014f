#!/usr/bin/env python3
"""Diagnostic: per-tile phase stamps of the fp32 producer/consumer step inside a grow, with the fire masks drawn beforehand (default)
and drawn in the kernel (ncahip_debug_force_generic bit 7, the kernel without FW) -- the producer's S3 in particular.

Needs a library whose csrc/nca_cond_pc.hip was compiled with -DNCA_STAMPS=2 (s_memtime stamps around the phases of stage_tile and
of the consumer's tile; never the shipped library), as video-stylization-with-nca_amd/libncahip_stamps2.so or the path in
NCAHIP_STAMPS_LIB.  bench.py's shape; the stamps of the grow's last step stay in the buffer.  The numbers are s_memtime ticks
(shader cycles), medians over all waves of the role and tiles 1..7 of each (tile 0 overlaps the weight-image fill).  The stamps
themselves cost cycles in every tile: compare the two columns, not their absolute values.
usage: python tools/stamp_fire.py > profiles/<tag>_phases.txt"""
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
        n = ops.fire_word_launches()
    finally:
        ops.force_generic(0)
    s = buf[:NWG * 8 * TILES * 16].cpu().numpy().reshape(NWG, 8, TILES, 16).astype(np.float64)
    cons, prod = s[:, 0:4, 1:], s[:, 4:8, 1:]
    med = lambda a: float(np.median(a))
    out = {"fire-word launches of the grow": n,
           "producer S1 (alpha' halo)           8 -> 9": med(prod[..., 9] - prod[..., 8]),
           "producer S2 (life, resolved alpha)  9 -> 10": med(prod[..., 10] - prod[..., 9]),
           "producer S3 (pre mask, fire list)  10 -> 11": med(prod[..., 11] - prod[..., 10]),
           "producer S4 (state, z, halo)       11 -> 13": med(prod[..., 13] - prod[..., 11]),
           "producer stage_tile                 8 -> 13": med(prod[..., 13] - prod[..., 8]),
           "producer tile period (8 -> next 8)": med(s[:, 4:8, 2:, 8] - s[:, 4:8, 1:-1, 8]),
           "consumer tile (first perception -> stored) 4 -> 8": med(cons[..., 8] - cons[..., 4]),
           "consumer tile period (4 -> next 4)": med(s[:, 0:4, 2:, 4] - s[:, 0:4, 1:-1, 4])}
    return out


a, b = run(0), run(128)
a2, b2 = run(0), run(128)
print("# tools/stamp_fire.py: s_memtime ticks (shader cycles), medians; fire words / in-kernel draw (bit 7), each measured twice")
print("%-52s %12s %12s %12s %12s" % ("", "words", "in-kernel", "words (2)", "in-kernel (2)"))
for k in a:
    print("%-52s %12.1f %12.1f %12.1f %12.1f" % (k, a[k], b[k], a2[k], b2[k]))
