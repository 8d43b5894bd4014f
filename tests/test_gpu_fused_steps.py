"""GPU tests of the fused-steps launches of a ConditionedNCA grow (MS in csrc/nca_cond_pc.hip, the driver in csrc/nca_capi.hip).

Where a grow draws its fire masks beforehand and the narrow-carve producer/consumer kernel walks at least two rounds per workgroup,
ncahip_cond_grow_fwd_f32 sends the steps of a chunk out as ONE launch: a tile of step t + 1 waits for its 3 x 3 neighbourhood of
4 x 16 tiles of step t through one counter per tile.  Contract: every bit of x_final, of the last pending ring slot and of every
pre slot equals the same grow with the off switch set (ncahip_debug_force_generic bit 24: one launch per step, the parent's code
path); ops.fused_step_launches() tells which path ran, and where the path does not apply it reads 0 and the results are still
those of the off switch."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_FUSED = 1 << 24        # ncahip_debug_force_generic bit 24: the off switch
ONE = 255                 # fire-word chunk cap (bits 16-23) that means "one chunk": it also waives the minimum grow length / grid size


def _bits(fw_cap=ONE, wg_cap=0, ms_cap=0):
    """hook word: fire-word chunk cap (bits 16-23), workgroup cap (bits 8-15), steps per fused launch (bits 25-27)"""
    return (fw_cap << 16) | (wg_cap << 8) | (ms_cap << 25)


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:          # the per-step / fused-steps kernels are under test
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


def _inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 0.5).to(DEV)
    goal = (torch.randn(B, C - 4, H, W, generator=g) * 0.5).to(DEV)
    return x, goal


def _grow(ops, bits, x, Tn, goal, w, ring, rate=0.5, seed=5, step0=0, us=None, x_final_slot=None):
    """ncahip_cond_grow_fwd_f32 itself with a ring of `ring` slots (pre zeroed: a slot no step writes compares equal).  x_final is a
    buffer of its own, or ring slot x_final_slot.  Returns clones of (x_final, last pending slot, every pre slot) and the fused-steps
    and fire-word launch counts."""
    from ncahip import _capi
    from ncahip.ops import _p, _stream, _u_args
    B, C, H, W = x.shape
    states = torch.empty(ring, B, C, H, W, device=DEV)
    pre = torch.zeros(ring, B, H, W, device=DEV, dtype=torch.uint8)
    states[0].copy_(x)
    x_final = torch.empty_like(x) if x_final_slot is None else states[x_final_slot]
    us, seed = _u_args(us, Tn, B, H, W, seed)
    ops.force_generic(bits)
    try:
        _capi.check(_capi.lib().ncahip_cond_grow_fwd_f32(_p(states), _p(pre), ring, Tn, _p(x_final), _p(goal), goal.shape[1], _p(us), _p(w.wp),
                                                         _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, 3, 0.1, rate,
                                                         -10.0, 10.0, seed, step0, _stream()), "cond_grow_fwd_f32")
        ops.check_errors()
        n_fused, n_words = ops.fused_step_launches(), ops.fire_word_launches()
    finally:
        ops.force_generic(0)
    last = None if x_final_slot == Tn % ring else states[Tn % ring].clone()
    return x_final.clone(), last, pre.clone(), n_fused, n_words


def _same(new, ref, tag):
    for k, name in enumerate(("x_final", "last pending slot")):
        if new[k] is None:
            continue
        a, b = new[k].view(torch.int32), ref[k].view(torch.int32)
        assert torch.equal(a, b), (tag, name, int((a != b).sum()))
        assert torch.equal(new[k], ref[k]), (tag, name)
    assert torch.equal(new[2], ref[2]), (tag, "pre slots", int((new[2] != ref[2]).sum()))


def _expected_launches(Tn, fw_cap, ms_cap, C):
    chunk = min(fw_cap, 32 * C - 1)          # words of the chunk + the counters fit x_final
    n, t = 0, 0
    while t < Tn:
        c = min(chunk, Tn - t)
        n += -(-c // ms_cap) if ms_cap else 1
        t += c
    return n


def _check(ops, x, goal, w, Tn, ring, fw_cap, wg_cap, ms_cap, **kw):
    bits = _bits(fw_cap, wg_cap, ms_cap)
    ref = _grow(ops, bits | NO_FUSED, x, Tn, goal, w, ring, **kw)
    assert ref[3] == 0 and ref[4] > 0, "the reference run takes the fire words, one launch per step"
    new = _grow(ops, bits, x, Tn, goal, w, ring, **kw)
    assert new[3] == _expected_launches(Tn, fw_cap, ms_cap, x.shape[1]) and new[3] > 0, ("fused launches", new[3])
    assert new[4] == ref[4]
    _same(new, ref, (tuple(x.shape), Tn, ring, fw_cap, wg_cap, ms_cap))
    assert bool(torch.isfinite(new[0]).all())
    return new


# C, hidden, B, H, W, workgroup cap, T, fire-word chunk cap, steps per fused launch, fire rate, ring (0: T + 1)
# 48 x 64 = 12 super-tiles per item, 16 x 32 = 2, 12 x 48 = 3 with H % 16 != 0 (pair 3 idle); capped to one or two workgroups a pair
# walks 3 - 36 rounds per step; T = 9 as one chunk and as 4 + 4 + 1
CASES = [(16, 64, 2, 48, 64, 1, 5, ONE, 0, 0.5, 2),
         (16, 64, 3, 48, 64, 2, 9, ONE, 0, 0.5, 2),
         (16, 64, 2, 48, 64, 2, 9, 4, 0, 0.5, 3),
         (16, 64, 3, 16, 32, 1, 9, 4, 2, 0.5, 3),
         (16, 64, 2, 12, 48, 2, 1, ONE, 0, 0.5, 2),
         (16, 64, 3, 12, 48, 1, 2, ONE, 0, 1.0, 3),
         (16, 64, 2, 48, 64, 5, 9, ONE, 3, 0.5, 2),      # five workgroups: uneven chunks of the tile list
         (12, 64, 3, 12, 48, 1, 5, ONE, 2, 0.5, 2),
         (12, 64, 2, 16, 32, 1, 2, ONE, 0, 1.0, 2),
         (12, 64, 3, 48, 64, 2, 9, 4, 3, 0.0, 0),
         (14, 64, 2, 48, 64, 2, 9, ONE, 3, 0.5, 0),
         (14, 64, 3, 16, 32, 2, 5, ONE, 1, 1.0, 2),
         (10, 48, 3, 16, 32, 2, 5, ONE, 1, 0.0, 2),
         (10, 48, 2, 48, 64, 1, 9, 4, 2, 0.5, 3),
         (10, 48, 3, 12, 48, 2, 2, ONE, 0, 0.5, 0)]


@pytest.mark.parametrize("C,hidden,B,H,W,wg_cap,Tn,fw_cap,ms_cap,rate,ring", CASES)
def test_fused_equals_one_launch_per_step(ops, C, hidden, B, H, W, wg_cap, Tn, fw_cap, ms_cap, rate, ring):
    x, goal = _inputs(B, C, H, W, 1)
    w = _w(ops, _prm(C, 1, hidden), x)
    _check(ops, x, goal, w, Tn, ring or Tn + 1, fw_cap, wg_cap, ms_cap, rate=rate, seed=5 | (3 << 32))


def test_step_counter_carries_into_its_high_word(ops):
    x, goal = _inputs(2, 16, 48, 64, 2)
    w = _w(ops, _prm(16, 2), x)
    _check(ops, x, goal, w, 9, 2, ONE, 2, 0, rate=0.5, seed=7, step0=2 ** 32 - 4)


def test_seed_grow(ops):
    """from the reference's seed state: most tiles are dead"""
    C, H, W = 16, 64, 64
    x = O.cond_generate_seed(2, C, 3, H).to(DEV)
    goal = (torch.randn(2, C - 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).to(DEV)
    w = _w(ops, _prm(C, 6), x)
    _check(ops, x, goal, w, 9, 10, ONE, 2, 0, rate=0.5, seed=13)


def test_grow_with_deaths(ops):
    """a sparse alpha channel: about half the cells start dead and cells die on the way (the pre masks cross tiles and steps)"""
    B, C, H, W, Tn = 2, 16, 48, 64, 9
    x, goal = _inputs(B, C, H, W, 8)
    x[:, 3] = (0.2 * (torch.rand(B, H, W, generator=torch.Generator().manual_seed(10)) < 0.08).float()).to(DEV)
    w = _w(ops, _prm(C, 8), x)
    out = _check(ops, x, goal, w, Tn, Tn + 1, ONE, 2, 0, rate=0.5, seed=17)
    pre = out[2].bool()
    assert bool((~pre[1]).any()) and bool(pre[1].any())
    assert any(bool((pre[t] & ~pre[t + 1]).any()) for t in range(1, Tn)), "no cell died"


def test_hardly_any_cell_fires(ops):
    """one workgroup, 96 rounds per step, a fire rate at which no carry group comes together within 64 tiles: the list of unpublished
    tiles fills up and the padded group runs early"""
    x, goal = _inputs(3, 16, 64, 128, 4)
    w = _w(ops, _prm(16, 4), x)
    _check(ops, x, goal, w, 3, 2, ONE, 1, 0, rate=0.004, seed=19)


def test_every_workgroup_of_the_device(ops):
    """no workgroup cap: 512 super-tiles, two rounds per workgroup on 256 CUs, every workgroup gated by others"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = -(-2 * cus // 256)
    x, goal = _inputs(B, 16, 256, 256, 11)
    w = _w(ops, _prm(16, 11), x)
    _check(ops, x, goal, w, 5, 2, ONE, 0, 0, rate=0.5, seed=29)


def test_bench_shape(ops):
    x, goal = _inputs(8, 16, 256, 256, 12)
    w = _w(ops, _prm(16, 12), x)
    _check(ops, x, goal, w, 8, 2, ONE, 0, 0, rate=0.5, seed=31)


def test_unhooked_long_grow_takes_the_path(ops):
    """no hook at all: the bench's grow (T x rounds >= 106) goes out as one fused launch"""
    x, goal = _inputs(8, 16, 256, 256, 13)
    w = _w(ops, _prm(16, 13), x)
    new = _grow(ops, 0, x, 16, goal, w, 2, seed=37)
    ref = _grow(ops, NO_FUSED, x, 16, goal, w, 2, seed=37)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rounds = -(-8 * 256 // cus)
    taken = rounds >= 2 and 16 * rounds >= 106
    assert new[3] == (1 if taken else 0) and ref[3] == 0
    _same(new, ref, "unhooked")


# ---- where the path must not be taken ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one round", "C20", "W20", "ring slot", "uniforms", "bit masks"])
def test_path_not_taken(ops, case):
    B, C, H, W, Tn, wg_cap, slot = 2, 16, 16, 32, 9, 1, None
    us = None
    if case == "one round":
        wg_cap = 0                               # four super-tiles, four workgroups
    elif case == "C20":
        C, H, W = 20, 48, 64
    elif case == "W20":
        W = 20
    elif case == "ring slot":
        slot = 1                                 # ring 3, T = 9: the last pending slot is slot 0
    x, goal = _inputs(B, C, H, W, 3)
    w = _w(ops, _prm(C, 3), x)
    if case in ("uniforms", "bit masks"):
        us = torch.rand(Tn, B, 1, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
        if case == "bit masks":
            us = ops.pack_fire_mask(us, 0.5, "cond")
    bits = _bits(ONE, wg_cap, 0)
    new = _grow(ops, bits, x, Tn, goal, w, 3, seed=21, us=us, x_final_slot=slot)
    ref = _grow(ops, bits | NO_FUSED, x, Tn, goal, w, 3, seed=21, us=us, x_final_slot=slot)
    assert new[3] == 0 and ref[3] == 0, "the path was taken"
    _same(new, ref, case)
    if case == "one round":                      # the same grid under a workgroup cap does take it
        assert _grow(ops, _bits(ONE, 1, 0), x, Tn, goal, w, 3, seed=21)[3] == 1
