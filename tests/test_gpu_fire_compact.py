"""GPU tests of the firing-cell lists of the fp32 producer/consumer ConditionedNCA step (csrc/nca_cond_pc.hip, FC): the consumer
runs perception and UpdateNet on the cells that fire only, and a cell that does not fire keeps its resolved state.  Contract:
the same values as the dense producer/consumer kernel (ncahip_debug_force_generic bit 5) and as the wave-private kernel
(bit 1, C <= 16), in the final state and in every history slot.  Bits may differ only in the sign of a zero (x + 0 * out with
x = -0 is +0 in the dense kernels, the kept -0 here)."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
DENSE, WAVE = 32, 2


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
        ops.check_errors()
    finally:
        ops.force_generic(0)
    return out


def _same(a, b, tag):
    assert torch.equal(a, b), tag
    ia, ib = a.view(torch.int32), b.view(torch.int32)
    diff = ia != ib
    assert bool((a[diff] == 0).all()) and bool((b[diff] == 0).all()), (tag, int(diff.sum()))


def _check(ops, x, Tn, goal, us, w, hist=True, wave=True, **kw):
    """compacting kernel vs dense producer/consumer (and wave-private) on the same inputs; returns the compacting result"""
    new = _grow(ops, 0, x, Tn, goal, us, w, 3, keep_history=hist, **kw)
    refs = [("dense", _grow(ops, DENSE, x, Tn, goal, us, w, 3, keep_history=hist, **kw))]
    if wave:
        refs.append(("wave", _grow(ops, WAVE, x, Tn, goal, us, w, 3, keep_history=hist, **kw)))
    for name, ref in refs:
        _same(new[0], ref[0], (name, "x_final"))
        if hist:
            for t in range(Tn + 1):
                _same(new[1][t], ref[1][t], (name, "states", t))
            for t in range(1, Tn + 1):                       # pre slot 0 is not written (the input has no pending mask)
                assert torch.equal(new[2][t], ref[2][t]), (name, "pre", t)
    assert bool(torch.isfinite(new[0]).all())
    return new


def _inputs(B, C, H, W, seed, gch=None):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 0.5).to(DEV)
    goal = (torch.randn(B, C - 4 if gch is None else gch, H, W, generator=g) * 0.5).to(DEV)
    return x, goal


def _us(ops, mode, Tn, B, H, W, rate, seed):
    if mode == "philox":
        return None
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(Tn, B, 1, H, W, generator=g).to(DEV)
    return u if mode == "uniform" else ops.pack_fire_mask(u, rate, "cond")


@pytest.mark.parametrize("mode", ["philox", "uniform", "bits"])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5, 0.9, 1.0])
def test_rates_and_masks(ops, rate, mode):
    """C = 16, 40 x 72: partial super-tiles in both directions (pairs 2-3 of the last row idle, a half-wide last column)"""
    B, C, H, W, Tn = 2, 16, 40, 72, 5
    x, goal = _inputs(B, C, H, W, 1)
    w = _w(ops, _prm(C, 1), x)
    _check(ops, x, Tn, goal, _us(ops, mode, Tn, B, H, W, rate, 2), w, fire_rate=rate, seed=5)


@pytest.mark.parametrize("C", [12, 20])
@pytest.mark.parametrize("mode", ["philox", "uniform", "bits"])
def test_channels(ops, C, mode):
    """C = 12 and the reference's default C = 20 (wide LDS carve; no wave-private kernel there)"""
    B, H, W, Tn = 2, 48, 52, 4
    x, goal = _inputs(B, C, H, W, 3)
    w = _w(ops, _prm(C, 3), x)
    _check(ops, x, Tn, goal, _us(ops, mode, Tn, B, H, W, 0.5, 4), w, wave=C <= 16, fire_rate=0.5, seed=9)


def test_batch_one_and_seed_grow(ops):
    """B = 1; a grow from the reference's seed (a mostly dead grid: most tiles stage, few cells change)"""
    C, H, W, Tn = 16, 64, 64, 12
    x = O.cond_generate_seed(1, C, 3, H).to(DEV)
    goal = (torch.randn(1, C - 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).to(DEV)
    w = _w(ops, _prm(C, 6), x)
    out = _check(ops, x, Tn, goal, None, w, fire_rate=0.5, seed=13)
    assert int((out[0][0, 3] > 0.1).sum()) > 1          # it grew


def test_hand_built_masks(ops):
    """Wave tiles (4 x 16 cells) that fire fully, not at all, in a checkerboard, with exactly 16 / 17 / 1 cells (group
    boundaries), and a random one, through explicit uniforms (0 fires, 1 never does at rate 0.5)."""
    B, C, H, W, Tn = 2, 16, 32, 48, 3
    x, goal = _inputs(B, C, H, W, 7)
    w = _w(ops, _prm(C, 7), x)
    u = torch.ones(Tn, B, 1, H, W)
    u[:, :, :, 0:4, 0:16] = 0.0                                                  # full
    ii, jj = torch.meshgrid(torch.arange(4), torch.arange(16), indexing="ij")
    u[:, :, :, 8:12, 0:16] = ((ii + jj) % 2).float()                             # checkerboard (32 cells)
    u[:, :, :, 12, 0:16] = 0.0                                                   # exactly 16
    t17 = torch.ones(64)
    t17[:17] = 0.0
    u[:, :, :, 0:4, 16:32] = t17.view(4, 16)                                     # 17 (in cell order)
    u[:, :, :, 4, 20] = 0.0                                                      # 1
    g = torch.Generator().manual_seed(8)
    u[:, :, :, 16:32, 32:48] = torch.rand(Tn, B, 1, 16, 16, generator=g)         # random
    u[:, 1, :, 20:24, 0:16] = 0.0                                                # batch 1: another full tile
    _check(ops, x, Tn, goal, u.to(DEV), w, fire_rate=0.5)


def test_bench_shape(ops):
    """The benchmark's grow: 8 x 16 x 256^2, 64 steps, in-kernel Philox at rate 0.5 (final state)"""
    B, C, H, W, Tn = 8, 16, 256, 256, 64
    x, goal = _inputs(B, C, H, W, 11)
    w = _w(ops, _prm(C, 11), x)
    _check(ops, x, Tn, goal, None, w, hist=False, fire_rate=0.5, seed=42)
