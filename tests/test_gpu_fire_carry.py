"""GPU tests of the carry of partial firing-cell groups across a pair's tiles in the fp32 producer/consumer ConditionedNCA step
(csrc/nca_cond_pc.hip, CARRY; C <= 16).  A consumer wave no longer pads a tile's last group of 16 MFMA columns: the cells of the
remainder get their perception, wait in the wave's carry, and UpdateNet runs on them once 16 have come together -- from whichever
tiles of the pair -- and once more after the pair's last round.  Contract: every cell gets the same bits as from the kernel that
pads every tile (ncahip_debug_force_generic bit 6), and the same values as the dense producer/consumer kernel (bit 5) and the
wave-private kernel (bit 1) up to the sign of a zero (see test_gpu_fire_compact.py), in the final state and every history slot.

The carry only crosses tiles when a workgroup has more than one round, so the grids here are small and bits 8-15 of the hook cap
the workgroup count: with 2 workgroups a 48 x 64 grid (3 x 4 super-tiles of 16 x 16) gives every pair 6 rounds, with 1 it gives 12.
Workgroup w of n then walks super-tiles w*12/n ... in order; pair p owns rows 4p..4p+3 of each."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOCARRY, DENSE, WAVE = 64, 32, 2


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:          # the per-step kernels are under test
        o.check_errors()
        yield o


def _prm(C, seed, hidden=64):
    g = torch.Generator().manual_seed(seed)
    return {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
            "update_net.out.0.weight": torch.randn(hidden, 3 * C, 1, 1, generator=g) * (1.0 / (3 * C) ** 0.5),
            "update_net.out.0.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.2.weight": torch.randn(hidden, hidden, 1, 1, generator=g) * (1.0 / hidden ** 0.5),
            "update_net.out.2.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.4.weight": torch.randn(C, hidden, 1, 1, generator=g) * (0.6 / hidden ** 0.5)}


def _w(ops, prm, like):
    return ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                           prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], like)


def _grow(ops, bits, *args, **kw):
    ops.force_generic(bits)
    try:
        out = ops.cond_grow(*args, **kw)
        out = tuple(None if r is None else r.clone() for r in out)
        ops.check_errors()                # the sticky error word is clear after every launch sequence
    finally:
        ops.force_generic(0)
    return out


def _bits_equal(a, b, tag):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, int((a.view(torch.int32) != b.view(torch.int32)).sum()))


def _same(a, b, tag):
    """equal values; bits may differ in the sign of a zero only (test_gpu_fire_compact.py)"""
    assert torch.equal(a, b), tag
    diff = a.view(torch.int32) != b.view(torch.int32)
    assert bool((a[diff] == 0).all()) and bool((b[diff] == 0).all()), (tag, int(diff.sum()))


def _check(ops, x, Tn, goal, us, w, cap, hist=True, wave=True, **kw):
    """the default (carry) kernel under a workgroup cap vs the padding list kernel (bits), dense and wave-private (values)"""
    cb = cap << 8
    new = _grow(ops, cb, x, Tn, goal, us, w, 3, keep_history=hist, **kw)
    refs = [("nocarry", _bits_equal, _grow(ops, cb | NOCARRY, x, Tn, goal, us, w, 3, keep_history=hist, **kw)),
            ("dense", _same, _grow(ops, cb | DENSE, x, Tn, goal, us, w, 3, keep_history=hist, **kw))]
    if wave:
        refs.append(("wave", _same, _grow(ops, WAVE, x, Tn, goal, us, w, 3, keep_history=hist, **kw)))
    for name, cmp, ref in refs:
        cmp(new[0], ref[0], (name, "x_final"))
        if hist:
            for t in range(Tn + 1):
                cmp(new[1][t], ref[1][t], (name, "states", t))
            for t in range(1, Tn + 1):                       # pre slot 0 is not written (the input has no pending mask)
                assert torch.equal(new[2][t], ref[2][t]), (name, "pre", t)
    assert bool(torch.isfinite(new[0]).all())
    return new


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 0.5).to(DEV)
    goal = (torch.randn(B, C - 4, H, W, generator=g) * 0.5).to(DEV)
    return x, goal


def _us(ops, mode, Tn, B, H, W, rate, seed):
    if mode == "philox":
        return None
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(Tn, B, 1, H, W, generator=g).to(DEV)
    return u if mode == "uniform" else ops.pack_fire_mask(u, rate, "cond")


SHAPES = [(1, 16, 64, 48, 64),      # C = 16 exact
          (1, 12, 64, 48, 64),      # C = 12 exact
          (1, 10, 48, 48, 64),      # CP = 12, padded channels and hidden units
          (1, 14, 64, 48, 64),      # CP = 16, padded channels
          (1, 16, 64, 40, 52),      # partial super-tiles in both directions (pairs 2-3 of the last row idle, a 4-wide last column)
          (3, 16, 64, 48, 64)]      # a carry whose cells belong to different batch items


@pytest.mark.parametrize("cap", [1, 2, 0])
@pytest.mark.parametrize("B,C,hidden,H,W", SHAPES)
def test_shapes(ops, B, C, hidden, H, W, cap):
    Tn = 3
    x, goal = _inputs(B, C, H, W, 1)
    w = _w(ops, _prm(C, 1, hidden), x)
    _check(ops, x, Tn, goal, None, w, cap, fire_rate=0.5, seed=5)


@pytest.mark.parametrize("mode", ["philox", "uniform", "bits"])
@pytest.mark.parametrize("rate", [0.0, 1.0, 0.5])
def test_rates_and_masks(ops, rate, mode):
    B, C, H, W, Tn = 1, 16, 48, 64, 3
    x, goal = _inputs(B, C, H, W, 2)
    w = _w(ops, _prm(C, 2), x)
    _check(ops, x, Tn, goal, _us(ops, mode, Tn, B, H, W, rate, 3), w, 2, fire_rate=rate, seed=7)


# Firing cells per wave tile, in the order a pair meets its tiles under a cap of 2 workgroups (6 rounds), one sequence per
# (workgroup, pair).  c = carry count before the tile, r = N mod 16:
SEQUENCES = [
    [16, 32, 0, 64, 48, 16],      # r = 0 on every tile: the carry is never used
    [7, 8, 1, 9, 8, 0],           # c + r = 15 (parks), then 16 (exactly full), 9, then 17 (one cell wraps), alive at the flush
    [0, 0, 16, 32, 0, 5],         # a carry alive only at the final flush
    [10, 0, 10, 64, 3, 12],       # N = 0 between two tiles with remainders; N = 64 with a carry alive
    [15, 15, 15, 15, 15, 15],     # every tile but the first wraps as many cells as it can
    [63, 63, 63, 1, 17, 33],      # full groups and a remainder in one tile
    [1, 1, 1, 1, 1, 1],           # only the flush runs UpdateNet
    [64, 64, 64, 64, 64, 64],
]


def _tile_mask(n, g):
    """a 4 x 16 wave tile of uniforms in which n cells, at random places, fire (0 fires, 1 never does at rate 0.5)"""
    t = torch.ones(64)
    t[torch.randperm(64, generator=g)[:n]] = 0.0
    return t.view(4, 16)


@pytest.mark.parametrize("mode", ["uniform", "bits"])
@pytest.mark.parametrize("cap", [2, 1])
def test_hand_built_masks(ops, cap, mode):
    """every carry boundary, forced through explicit masks (the same every step); under a cap of 1 the two workgroups' sequences
    follow each other in one carry"""
    B, C, H, W, Tn = 1, 16, 48, 64, 2
    x, goal = _inputs(B, C, H, W, 4)
    w = _w(ops, _prm(C, 4), x)
    g = torch.Generator().manual_seed(9)
    u = torch.ones(H, W)
    for wg in range(2):
        for pair in range(4):
            for k, n in enumerate(SEQUENCES[4 * wg + pair]):
                st = 6 * wg + k                              # super-tile: 4 per row of super-tiles
                y0, x0 = 16 * (st // 4) + 4 * pair, 16 * (st % 4)
                u[y0:y0 + 4, x0:x0 + 16] = _tile_mask(n, g)
    us = u.expand(Tn, B, 1, H, W).contiguous().to(DEV)
    if mode == "bits":
        us = ops.pack_fire_mask(us, 0.5, "cond")
    _check(ops, x, Tn, goal, us, w, cap, fire_rate=0.5)


def test_seed_grow(ops):
    """6 steps with history from the reference's seed state (a mostly dead grid), 8 rounds per pair"""
    C, H, W, Tn = 16, 64, 64, 6
    x = O.cond_generate_seed(1, C, 3, H).to(DEV)
    goal = (torch.randn(1, C - 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).to(DEV)
    w = _w(ops, _prm(C, 6), x)
    _check(ops, x, Tn, goal, None, w, 2, fire_rate=0.5, seed=13)


def test_grow_with_deaths(ops):
    """a sparse alpha channel: about half the cells start dead and cells die on the way -- dead cells are in the lists all the same"""
    B, C, H, W, Tn = 1, 16, 48, 64, 6
    x, goal = _inputs(B, C, H, W, 8)
    g = torch.Generator().manual_seed(10)
    x[:, 3] = (0.2 * (torch.rand(B, H, W, generator=g) < 0.08).float()).to(DEV)
    w = _w(ops, _prm(C, 8), x)
    out = _check(ops, x, Tn, goal, None, w, 2, fire_rate=0.5, seed=17)
    pre = out[2].bool()
    assert bool((~pre[1]).any()) and bool(pre[1].any())
    assert any(bool((pre[t] & ~pre[t + 1]).any()) for t in range(1, Tn)), "no cell died"


def test_c20_dispatch(ops):
    """C = 20 (wide carve) has no carry: bit 6 selects the same kernel, the outputs are the same bits"""
    B, C, H, W, Tn = 1, 20, 48, 64, 3
    x, goal = _inputs(B, C, H, W, 12)
    w = _w(ops, _prm(C, 12), x)
    a = _grow(ops, 2 << 8, x, Tn, goal, None, w, 3, keep_history=True, fire_rate=0.5, seed=3)
    b = _grow(ops, (2 << 8) | NOCARRY, x, Tn, goal, None, w, 3, keep_history=True, fire_rate=0.5, seed=3)
    _bits_equal(a[0], b[0], "x_final")
    _bits_equal(a[1], b[1], "states")
    assert torch.equal(a[2][1:], b[2][1:])
