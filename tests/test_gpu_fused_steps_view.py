"""GPU tests of the fused-steps launch's step view and early gate (MS in csrc/nca_cond_pc.hip).

The fused launch keeps two scalars per wave -- the step of the launch and the ring index of its input slot -- and forms x_in, pre_in,
x_out, pre_out and the step's fire words from them and the launch's arguments where a tile needs them; the producer takes its first
look at a tile's nine counters before it waits for the tile buffer and polls only if that look came back closed.  Contract, as in
tests/test_gpu_fused_steps.py: every bit of x_final, of the last pending ring slot and of every pre slot equals the same grow with
the off switch set (ncahip_debug_force_generic bit 24: one launch per step), ops.fused_step_launches() > 0 says the path ran, and
ops.check_errors() is clean after every grow."""
import pytest
import torch

from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_FUSED = 1 << 24        # ncahip_debug_force_generic bit 24: the off switch
ONE = 255                 # fire-word chunk cap (bits 16-23) that means "one chunk"


def _bits(fw_cap=ONE, wg_cap=0, ms_cap=0):
    """hook word: fire-word chunk cap (bits 16-23), workgroup cap (bits 8-15), steps per fused launch (bits 25-27)"""
    return (fw_cap << 16) | (wg_cap << 8) | (ms_cap << 25)


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:
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


def _grow(ops, bits, x, Tn, goal, w, ring, rate=0.5, seed=5, step0=0):
    """ncahip_cond_grow_fwd_f32 itself with a ring of `ring` slots (pre zeroed: a slot no step writes compares equal).  Returns clones
    of (x_final, last pending slot, every pre slot) and the fused-steps and fire-word launch counts."""
    from ncahip import _capi
    from ncahip.ops import _p, _stream, _u_args
    B, C, H, W = x.shape
    states = torch.empty(ring, B, C, H, W, device=DEV)
    pre = torch.zeros(ring, B, H, W, device=DEV, dtype=torch.uint8)
    states[0].copy_(x)
    x_final = torch.empty_like(x)
    us, seed = _u_args(None, Tn, B, H, W, seed)
    ops.force_generic(bits)
    try:
        _capi.check(_capi.lib().ncahip_cond_grow_fwd_f32(_p(states), _p(pre), ring, Tn, _p(x_final), _p(goal), goal.shape[1], _p(us), _p(w.wp),
                                                         _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, 3, 0.1, rate,
                                                         -10.0, 10.0, seed, step0, _stream()), "cond_grow_fwd_f32")
        ops.check_errors()
        n_fused, n_words = ops.fused_step_launches(), ops.fire_word_launches()
    finally:
        ops.force_generic(0)
    return x_final.clone(), states[Tn % ring].clone(), pre.clone(), n_fused, n_words


def _same(new, ref, tag):
    for k, name in enumerate(("x_final", "last pending slot")):
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


# ---- view derivation --------------------------------------------------------------------------------------------------------
# B x C x H x W (hidden): the exact CP = 16 kernel, the exact CP = 12 kernel, and the padded EXACT = false twin of CP = 16
# (C = 14).  Under a workgroup cap of 2 a workgroup walks 2 - 18 rounds per step.
SHAPES = [(2, 16, 16, 32, 64), (3, 12, 48, 64, 64), (2, 14, 12, 48, 64)]
STEP0 = 2 ** 32 - 3       # the step counter carries into its high word inside the grow, and with it the fire-word offset


@pytest.mark.parametrize("B,C,H,W,hidden", SHAPES)
@pytest.mark.parametrize("Tn", [7, 9])
@pytest.mark.parametrize("ring", [2, 3, 0])            # 0: T + 1
@pytest.mark.parametrize("ms_cap", [1, 2, 3])
@pytest.mark.parametrize("fw_cap", [ONE, 4])           # one chunk; 4 + 4 + 1 (4 + 3 at T = 7): launches that start at t0 > 0
def test_view_of_every_step(ops, B, C, H, W, hidden, Tn, ring, ms_cap, fw_cap):
    """ms_t0 takes every residue modulo the ring, a ring wrap falls inside a launch (caps 2 and 3 on rings 2 and 3), the grow's step 0
    (no pending mask) runs inside a fused launch and later launches start at t0 > 0"""
    x, goal = _inputs(B, C, H, W, 21)
    w = _w(ops, _prm(C, 21, hidden), x)
    _check(ops, x, goal, w, Tn, ring or Tn + 1, fw_cap, 2, ms_cap, rate=0.5, seed=41, step0=STEP0)


@pytest.mark.parametrize("B,C,H,W,hidden", SHAPES)
@pytest.mark.parametrize("ring", [2, 3, 0])
def test_view_uncapped_launch(ops, B, C, H, W, hidden, ring):
    """no cap on the steps per launch: all 9 steps, and several ring wraps, in one launch"""
    x, goal = _inputs(B, C, H, W, 22)
    w = _w(ops, _prm(C, 22, hidden), x)
    _check(ops, x, goal, w, 9, ring or 10, ONE, 1, 0, rate=0.5, seed=43, step0=STEP0)


# ---- early gate -------------------------------------------------------------------------------------------------------------
# 48 x 64 = 12 super-tiles per item: with B = 1 one workgroup walks 12 rounds per step and two walk 6, and a step's first tiles wait
# for the previous step's last ones -- the early look comes back closed and the poll loop takes over
@pytest.mark.parametrize("wg_cap", [1, 2])
@pytest.mark.parametrize("rate", [0.0, 0.004, 0.5, 1.0])
def test_early_look_closed(ops, wg_cap, rate):
    """rates 0 and 0.004: no carry group comes together, tiles are published only at the end of a step"""
    x, goal = _inputs(1, 16, 48, 64, 23)
    w = _w(ops, _prm(16, 23), x)
    _check(ops, x, goal, w, 5, 2, ONE, wg_cap, 0, rate=rate, seed=47)


@pytest.mark.parametrize("wg_cap", [1, 2])
def test_early_look_with_deaths(ops, wg_cap):
    """a sparse alpha channel: cells die on the way, the pre masks cross tiles and steps"""
    B, C, H, W, Tn = 2, 16, 48, 64, 9
    x, goal = _inputs(B, C, H, W, 8)
    x[:, 3] = (0.2 * (torch.rand(B, H, W, generator=torch.Generator().manual_seed(10)) < 0.08).float()).to(DEV)
    w = _w(ops, _prm(C, 8), x)
    out = _check(ops, x, goal, w, Tn, Tn + 1, ONE, wg_cap, 0, rate=0.5, seed=17)
    pre = out[2].bool()                      # ring T + 1: slot t holds the mask step t - 1 wrote
    assert bool((~pre[1]).any()) and bool(pre[1].any())
    assert any(bool((pre[t] & ~pre[t + 1]).any()) for t in range(1, Tn)), "no cell died"
