"""GPU tests of a ConditionedNCA grow's fire masks drawn before its steps (csrc/nca_cond_fire.hip; FW in csrc/nca_cond_pc.hip).

ncahip_cond_fire_words writes, for a chunk of steps, one 64-bit word per 4 x 16 tile: bit 16 * row + col <=> the cell fires, by
the step kernels' own predicate on the same Philox stream.  ncahip_cond_grow_fwd_f32 draws them into x_final (dead until the
finalize) and its producer waves read the word instead of drawing.  Contract: the words equal the per-cell draw
(ops.philox_uniform) under the same clamp and compare, bit for bit; a grow on the words equals the grow whose steps draw in the
kernel (ncahip_debug_force_generic bit 7: the parent's code path) in every bit of the final state, the pre masks and the history;
and where the path does not apply (shape, scratch, mask source, length) the grow falls back, observably
(ops.fire_word_launches() == 0), to the same results."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF = 128                 # ncahip_debug_force_generic bit 7: the steps draw their masks themselves
MIN_ROUNDS, MIN_STEP_ROUNDS = 2, 106   # fire_words_pay (csrc/nca_capi.hip): a grow draws beforehand only on a grid that gives a step
#                                        launch's workgroups >= 2 super-tiles each, and only with T x that number >= 106 ...
ONE = 255 << 16           # ... unless a chunk cap is set (bits 16-23): the small grids and T = 9 of these tests, as one chunk


def _cap(n):
    return n << 16        # bits 16-23: at most n steps per fire-word launch


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:          # the per-step kernels are under test
        o.check_errors()
        yield o


# ---- the words against the per-cell draw ---------------------------------------------------------------------------------
def _expected_bits(ops, Tc, B, H, W, rate, seed, step0):
    """[Tc, B, H/4, W/16, 64] bool from ops.philox_uniform: clamp(u, 0, 1) < rate in float32, in the words' tile / lane order"""
    r = torch.tensor(rate, dtype=torch.float32, device=DEV)
    out = []
    for t in range(Tc):
        u = ops.philox_uniform(B, H, W, seed, step0 + t, device=DEV)[:, 0]
        fires = u.clamp(0.0, 1.0) < r
        out.append(fires.view(B, H // 4, 4, W // 16, 16).permute(0, 1, 3, 2, 4).reshape(B, H // 4, W // 16, 64))
    return torch.stack(out)


def _unpack(words):
    k = torch.arange(64, device=words.device, dtype=torch.int64)
    return ((words.unsqueeze(-1) >> k) & 1).bool()


BOUNDARY = 5000001 / 2 ** 24                                                  # rate * 2^24 is an integer: u == rate does not fire
ABOVE = float(torch.nextafter(torch.tensor(BOUNDARY, dtype=torch.float32), torch.tensor(1.0)))   # ... and just above it does
WORD_SHAPES = [(1, 4, 16), (3, 12, 48), (2, 8, 32)]
SEED_LO, SEED_HI = 0x1234, 0x1234 | (7 << 32)                                 # differ in the high word only


@pytest.mark.parametrize("Tc", [1, 3])
@pytest.mark.parametrize("step0", [0, 2 ** 32 + 5])
@pytest.mark.parametrize("B,H,W", WORD_SHAPES)
def test_words_equal_the_cell_draw(ops, B, H, W, step0, Tc):
    seen = {}
    for seed in (SEED_LO, SEED_HI):
        for rate in (0.0, 0.5, 1.0, BOUNDARY, ABOVE):
            words = ops.cond_fire_words(Tc, B, H, W, rate, seed, step0, device=DEV)
            assert words.shape == (Tc, B, H // 4, W // 16) and words.dtype == torch.int64
            got, want = _unpack(words), _expected_bits(ops, Tc, B, H, W, rate, seed, step0)
            assert torch.equal(got, want), (seed, rate, int((got != want).sum()))
            if rate == 0.0:
                assert not bool(got.any())
            if rate == 1.0:
                assert bool(got.all())
            if rate == 0.5:
                seen[seed] = words.clone()
                assert 0.3 < float(got.float().mean()) < 0.7
    assert not torch.equal(seen[SEED_LO], seen[SEED_HI]), "the seed's high word does not reach the key"


def test_words_steps_are_the_stream(ops):
    """step t of a chunk is step step0 + t of the stream; a high counter word is not the low one"""
    B, H, W = 2, 8, 32
    three = ops.cond_fire_words(3, B, H, W, 0.5, 9, 2 ** 32 + 5, device=DEV)
    for t in range(3):
        assert torch.equal(three[t], ops.cond_fire_words(1, B, H, W, 0.5, 9, 2 ** 32 + 5 + t, device=DEV)[0])
    assert not torch.equal(three[0], ops.cond_fire_words(1, B, H, W, 0.5, 9, 5, device=DEV)[0])


# ---- the grow on the words against the grow that draws in the kernel ------------------------------------------------------
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


def _grow(ops, bits, *args, **kw):
    """(x_final, states, pre, fire-word launches) of ops.cond_grow under the hook bits"""
    ops.force_generic(bits)
    try:
        out = ops.cond_grow(*args, **kw)
        out = tuple(None if r is None else r.clone() for r in out)
        ops.check_errors()
        n = ops.fire_word_launches()
    finally:
        ops.force_generic(0)
    return out + (n,)


def _bits_equal(a, b, tag):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (tag, int((a.view(torch.int32) != b.view(torch.int32)).sum()))


def _same_run(new, ref, Tn, hist, tag):
    _bits_equal(new[0], ref[0], (tag, "x_final"))
    assert torch.equal(new[0], ref[0])
    if hist:
        for t in range(Tn + 1):
            _bits_equal(new[1][t], ref[1][t], (tag, "states", t))
        for t in range(1, Tn + 1):                           # pre slot 0 is not written (the input has no pending mask)
            assert torch.equal(new[2][t], ref[2][t]), (tag, "pre", t)
    else:                                                    # ring 2: the last state slot and its pre mask
        _bits_equal(new[1][Tn % 2], ref[1][Tn % 2], (tag, "last state"))
        assert torch.equal(new[2][Tn % 2], ref[2][Tn % 2]), (tag, "pre")


def _check(ops, x, Tn, goal, w, hist, **kw):
    """one fire-word launch, and chunks of 4 (4 + 4 + 1 at T = 9: step0 of later chunks), against bit 7"""
    ref = _grow(ops, OFF, x, Tn, goal, None, w, 3, keep_history=hist, **kw)
    assert ref[3] == 0
    new = _grow(ops, ONE, x, Tn, goal, None, w, 3, keep_history=hist, **kw)
    assert new[3] == 1, "the grow did not draw its masks beforehand"
    _same_run(new, ref, Tn, hist, "one chunk")
    chunked = _grow(ops, _cap(4), x, Tn, goal, None, w, 3, keep_history=hist, **kw)
    assert chunked[3] == (Tn + 3) // 4
    _same_run(chunked, ref, Tn, hist, "chunks of 4")
    assert bool(torch.isfinite(new[0]).all())
    return new


GROW_SHAPES = [(2, 16, 64, 16, 32),      # C = 16 exact (the carry)
               (3, 12, 64, 12, 48),      # C = 12 exact; H not a multiple of the 16-row super-tile: pair 3 idle
               (2, 20, 64, 48, 64),      # C = 20, the wide carve (no carry)
               (3, 14, 64, 48, 64),      # CP = 16, padded channels
               (2, 10, 48, 16, 32),      # CP = 12, padded channels and hidden units
               (3, 18, 64, 12, 48)]      # CP = 20, padded channels


@pytest.mark.parametrize("hist", [False, True])
@pytest.mark.parametrize("B,C,hidden,H,W", GROW_SHAPES)
def test_grow_equals_in_kernel_draw(ops, B, C, hidden, H, W, hist):
    Tn = 9
    x, goal = _inputs(B, C, H, W, 1)
    w = _w(ops, _prm(C, 1, hidden), x)
    _check(ops, x, Tn, goal, w, hist, fire_rate=0.5, seed=5 | (3 << 32), step0=2 ** 32 - 4)   # the step counter carries into its high word


def test_seed_grow(ops):
    """9 steps with history from the reference's seed state (a mostly dead grid)"""
    C, H, W, Tn = 16, 64, 64, 9
    x = O.cond_generate_seed(2, C, 3, H).to(DEV)
    goal = (torch.randn(2, C - 4, H, W, generator=torch.Generator().manual_seed(6)) * 0.5).to(DEV)
    w = _w(ops, _prm(C, 6), x)
    _check(ops, x, Tn, goal, w, True, fire_rate=0.5, seed=13)


def test_grow_with_deaths(ops):
    """a sparse alpha channel: about half the cells start dead and cells die on the way"""
    B, C, H, W, Tn = 2, 16, 48, 64, 9
    x, goal = _inputs(B, C, H, W, 8)
    g = torch.Generator().manual_seed(10)
    x[:, 3] = (0.2 * (torch.rand(B, H, W, generator=g) < 0.08).float()).to(DEV)
    w = _w(ops, _prm(C, 8), x)
    out = _check(ops, x, Tn, goal, w, True, fire_rate=0.5, seed=17)
    pre = out[2].bool()
    assert bool((~pre[1]).any()) and bool(pre[1].any())
    assert any(bool((pre[t] & ~pre[t + 1]).any()) for t in range(1, Tn)), "no cell died"


# ---- fallbacks: taken, and right ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["W20", "uniforms", "bit masks"])
def test_fallback_through_ops(ops, case):
    """the chunk cap waives the length / grid rule, so each of these falls back for its own reason"""
    B, C, H, W, Tn = 2, 16, 16, 32, 9
    us = None
    if case == "W20":
        W = 20
    x, goal = _inputs(B, C, H, W, 3)
    w = _w(ops, _prm(C, 3), x)
    if case in ("uniforms", "bit masks"):
        us = torch.rand(Tn, B, 1, H, W, generator=torch.Generator().manual_seed(4)).to(DEV)
        if case == "bit masks":
            us = ops.pack_fire_mask(us, 0.5, "cond")
    new = _grow(ops, ONE, x, Tn, goal, us, w, 3, keep_history=True, fire_rate=0.5, seed=21)
    ref = _grow(ops, OFF, x, Tn, goal, us, w, 3, keep_history=True, fire_rate=0.5, seed=21)
    assert new[3] == 0 and ref[3] == 0, "the fallback was not taken"
    _same_run(new, ref, Tn, True, case)


def test_fallback_below_the_minimum_length(ops):
    """no hook: a grid of two super-tiles per workgroup draws beforehand from T = 106 / 2 on, not below"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    C, H, W = 16, 256, 256
    B = -(-MIN_ROUNDS * cus // 256)                          # 256 super-tiles per batch item
    rounds = -(-B * 256 // cus)
    t_min = -(-MIN_STEP_ROUNDS // rounds)
    x, goal = _inputs(B, C, H, W, 7)
    w = _w(ops, _prm(C, 7), x)
    short = _grow(ops, 0, x, t_min - 1, goal, None, w, 3, fire_rate=0.5, seed=23)
    ref = _grow(ops, OFF, x, t_min - 1, goal, None, w, 3, fire_rate=0.5, seed=23)
    assert short[3] == 0 and ref[3] == 0, "the fallback was not taken"
    _same_run(short, ref, t_min - 1, False, "short")
    taken = _grow(ops, 0, x, t_min, goal, None, w, 3, fire_rate=0.5, seed=23)     # one step more and the path is taken, unhooked
    ref = _grow(ops, OFF, x, t_min, goal, None, w, 3, fire_rate=0.5, seed=23)
    assert taken[3] == 1 and ref[3] == 0
    _same_run(taken, ref, t_min, False, "long enough")


def test_fallback_on_a_grid_of_one_round(ops):
    """no hook: one super-tile per workgroup never draws beforehand, however long the grow"""
    B, C, H, W, Tn = 2, 16, 16, 32, MIN_STEP_ROUNDS + 4
    x, goal = _inputs(B, C, H, W, 9)
    w = _w(ops, _prm(C, 9), x)
    new = _grow(ops, 0, x, Tn, goal, None, w, 3, fire_rate=0.5, seed=25)
    ref = _grow(ops, OFF, x, Tn, goal, None, w, 3, fire_rate=0.5, seed=25)
    assert new[3] == 0 and ref[3] == 0, "the fallback was not taken"
    _same_run(new, ref, Tn, False, "one round")


def _raw_grow(ops, bits, x, Tn, w, layout, seed):
    """ncahip_cond_grow_fwd_f32 itself, ring = T + 1, with an x_final that is (layout) a buffer of its own, slot 0 of the ring, or
    a range that overlaps the goal tensor.  Returns (x_final, states 1.., pre 1.., launches) as clones."""
    from ncahip import _capi
    from ncahip.ops import _p, _stream
    B, C, H, W = x.shape
    gch = C - 4
    n, ng = x.numel(), B * gch * H * W
    g = torch.Generator().manual_seed(31)
    goal_vals = (torch.randn(B, gch, H, W, generator=g) * 0.5).to(DEV)
    buf = torch.zeros(ng + n, device=DEV)                    # the goal, with room behind it
    goal = buf[:ng].view(B, gch, H, W)
    goal.copy_(goal_vals)
    states = torch.empty(Tn + 1, B, C, H, W, device=DEV)
    pre = torch.zeros(Tn + 1, B, H, W, device=DEV, dtype=torch.uint8)
    states[0].copy_(x)
    own = torch.empty_like(x)
    x_final = {"own": own, "ring slot": states[0], "goal": buf[ng // 2: ng // 2 + n]}[layout]
    assert x_final.data_ptr() % 16 == 0
    ops.force_generic(bits)
    try:
        _capi.check(_capi.lib().ncahip_cond_grow_fwd_f32(_p(states), _p(pre), Tn + 1, Tn, _p(x_final), _p(goal), gch, None, _p(w.wp), _p(w.w1),
                                                         _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, 3, 0.1, 0.5, -10.0, 10.0,
                                                         seed, 0, _stream()), "cond_grow_fwd_f32")
        ops.check_errors()
        n_launch = ops.fire_word_launches()
    finally:
        ops.force_generic(0)
    return x_final.reshape(B, C, H, W).clone(), states[1:].clone(), pre[1:].clone(), n_launch


@pytest.mark.parametrize("layout", ["ring slot", "goal"])
def test_fallback_when_x_final_is_no_scratch(ops, layout):
    B, C, H, W, Tn = 2, 16, 16, 32, 9
    x, _ = _inputs(B, C, H, W, 5)
    w = _w(ops, _prm(C, 5), x)
    taken = _raw_grow(ops, ONE, x, Tn, w, "own", 41)
    assert taken[3] == 1, "the reference run of this test does draw beforehand"
    new = _raw_grow(ops, ONE, x, Tn, w, layout, 41)
    ref = _raw_grow(ops, OFF, x, Tn, w, layout, 41)
    assert new[3] == 0 and ref[3] == 0, "the fallback was not taken"
    for k, name in enumerate(("x_final", "states", "pre")):
        assert torch.equal(new[k], ref[k]), (layout, name)
        assert torch.equal(new[k], taken[k]), (layout, name, "against the run on the words")
