"""The opt-in bf16-MFMA DyNCA step (ops.dynca_precision('bf16'), ncahip_dynca_precision mode 1) against float64 at the smallest shape
of every class it dispatches to: the sibling of test_gpu_dynca_b16_ref.py for the mode's own instantiations --

  per-step    {DyncaFwdBf, DyncaFwdMsBf} x {<12,96>, <16,128>} x {HAS_COND} x {VEC, any-shape}                  16 kernels
  steered     DyncaSteered<> of the same 16
  persistent  launch_cfg<MS, CP, FC, HAS_COND, true> (dynca_persist_kernel / dynca_persist_ms_kernel, BF = true)     8 kernels

Reference and caps: test_dynca_bf16_host.py, unchanged (the float64 restatement of the contract, the first-order bound E, cap (a)
|d| <= E (1 + 2^-7) elementwise, cap (b) at most FLIP_FRACTION of the elements beyond FLIP_TOL).  Rows, the instantiation each
reaches, batches (B = ceil(1024 / (H W)): cap (b) needs cells to count over), literal seeds and the CPU proof that the float64
restatement and an fp32 evaluation of the same contract agree within HALF of cap (b) on every (row, pad):
test_dynca_bf16_ref_host.py.  Every run here has the persistent kernel off unless it says otherwise.

  1  teacher-forced replay, every (row, pad), T = 3: states[t + 1] against contract_step(states[t]) through check_caps; cells whose
     mask is 0 keep their bits.  The rows of the persistent kernels are held to it as well.
  2  closeness to the exact step at step 0: within E of the float64 oracle step, elementwise; the same call under 'f32' differs
     bit-wise and is within REPLAY_TOL of the oracle -- the mode really ran.
  3  mask sources: in-kernel Philox and ops.pack_fire_mask words equal the explicit-uniform run bit for bit.
  4  forms agree: at W % 4 == 0 an input one float off 16-byte alignment takes the any-shape kernel and equals the VEC result bit
     for bit.  The two forms differ only in how they stage the state tile into LDS (TilePos::init<VEC>, pos_load); the perception
     sums are read from that tile by the same code in the same order, and both call the one NcaDyncaBf16::mlp.
  5  steered instantiations: an identity direction field attached equals the unattached call bit for bit.
  6  persistent kernels: the one-launch result equals the per-step result bit for bit and differs from 'f32'.
  7  range edge: (16, 128) is in the mode's range, (17, 128) and (16, 129) are not; a (16, 129) call under the mode is the fp32 call.

Every test prints its figures (-s); the last one prints the worst |d| / E and the worst cap-(b) fraction per class."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_dynca_bf16_host import FLIP_FRACTION, bf16_inputs, check_caps, contract_step
from test_dynca_bf16_ref_host import (PERSIST_ROWS, ROW_PADS, ROWS, SINGLE, TWO, admits, bf16_class, bf16_form, geometry,
                                      make_inputs, scales_of)
from util import REPLAY_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TN = 3
RATE = 0.5
PHILOX_SEED, PHILOX_STEP0 = 0x5EED0003, 7


def _id(v):
    return v if isinstance(v, str) else ("two_scale" if v else "single")


def one_pad(two, row):
    """one pad mode per row for the checks that compare two runs of the kernels with each other: the modes take turns over the rows"""
    pads = [p for p in O.PAD_MODES if admits(two, row, p)]
    return pads[(ROWS + PERSIST_ROWS).index((two, row)) % len(pads)]


ROW_ONE_PAD = [(two, row, one_pad(two, row)) for two, row in ROWS]
VEC_ROW_PADS = [(two, row, pad) for two, row, pad in ROW_PADS if (two, row) in ROWS and geometry(two, row)[5] % 4 == 0]
PERSIST_ROW_PADS = [(two, row, pad) for two, row, pad in ROW_PADS if (two, row) in PERSIST_ROWS]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=False) as o:
        yield o
        assert o.set_dynca_precision("f32") == "f32"


@pytest.fixture(autouse=True)
def _after_each(ops):
    yield
    ops.persistent_steps = False
    assert ops.set_dynca_precision("f32") == "f32"           # the test left the mode as it found it
    ops.check_errors()


def _weights(ops, prm, x):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def reaches(two, row):
    """(two_scale, class, HAS_COND, form) of a row's per-step run"""
    C, fc, cc, _, H, W = geometry(two, row)
    return two, bf16_class(C, fc), cc > 0, bf16_form(H, W)


_RUNS = {}
_WORST = {}      # reaches() -> [worst |d| / E, worst cap-(b) fraction, the (row, pad, step) of each]


def run(ops, two, row, pad):
    """inputs and the kept bf16-mode history (T = 3, explicit uniforms, per-step kernels) of one (row, pad): computed once, shared,
    left unchanged"""
    key = (two, row, pad)
    if key not in _RUNS:
        prm, x, cond, us = make_inputs(two, row, pad, device=DEV)
        w = _weights(ops, prm, x)
        with ops.dynca_precision("bf16"):
            out, states = ops.dynca_nsteps(x, TN, cond, us[:TN], w, pad, RATE, keep_history=True, two_scale=two)
        ops.check_errors()
        assert states.shape == (TN + 1,) + tuple(x.shape) and same_bits(states[0], x) and same_bits(states[TN], out)
        _RUNS[key] = dict(prm=prm, x=x, cond=cond, us=us, w=w, states=states.clone())
    return _RUNS[key]


def history(ops, r, two, pad, us, **kw):
    """the same call as run()'s with other masks or another ambient state; the stored states"""
    return ops.dynca_nsteps(r["x"], TN, r["cond"], us, r["w"], pad, RATE, keep_history=True, two_scale=two, **kw)[1]


# ================================================================================================ 1. teacher-forced replay
@pytest.mark.parametrize("two,row,pad", ROW_PADS, ids=_id)
def test_teacher_forced_replay(ops, two, row, pad):
    """every stored step against the restatement applied to the kernel's own previous state; idle cells keep their bits"""
    r = run(ops, two, row, pad)
    states, us = r["states"], r["us"]
    cls = reaches(two, row)
    worst = _WORST.setdefault(cls, [0.0, 0.0, None, None])
    for t in range(TN):
        ref, E = contract_step(states[t], r["cond"], us[t], r["prm"], pad, scales=scales_of(two))
        ratio, frac = check_caps(states[t + 1], ref, E, states[t], f"{_id(two)} {row} {geometry(two, row)} {pad} {cls[1:]} step {t}")
        if ratio > worst[0]:
            worst[0], worst[2] = ratio, (row, pad, t)
        if frac > worst[1]:
            worst[1], worst[3] = frac, (row, pad, t)
        idle = ((us[t] + RATE).floor() == 0).expand_as(states[t])
        assert torch.equal(states[t + 1].view(torch.int32)[idle], states[t].view(torch.int32)[idle]), (row, pad, t)
        assert bool(idle.any()) and not bool(idle.all())


# ================================================================================================ 2. closeness to the exact step
@pytest.mark.parametrize("two,row,pad", [k for k in ROW_PADS if k[:2] in ROWS], ids=_id)
def test_step_zero_is_within_E_of_the_exact_step_and_the_mode_ran(ops, two, row, pad):
    r = run(ops, two, row, pad)
    x, cond, u, prm = r["x"], r["cond"], r["us"][0], r["prm"]
    p64 = {k: v.double() for k, v in prm.items()}
    exact = O.dynca_step(x.double(), None if cond is None else cond.double(), u, p64, pad, RATE, scales_of(two))
    _, E = contract_step(x, cond, u, prm, pad, scales=scales_of(two))
    got = r["states"][1]
    d = (got.double() - exact).abs()
    ratio = float((d / E.clamp_min(1e-30))[E > 0].max())
    f32 = ops.dynca_nsteps(x, 1, cond, r["us"][:1], r["w"], pad, RATE, keep_history=True, two_scale=two)[1][1]
    e32 = rel_err(f32, exact)
    print(f"{_id(two)} {row} {pad}: |bf16 step - exact step| / E {ratio:.3f} (bound 1), fp32 kernel against the exact step {e32:.2e} "
          f"(bound {REPLAY_TOL:g}), elements the mode changes {int((f32 != got).sum())} of {got.numel()}")
    assert bool((d <= E).all()), ratio
    assert not same_bits(f32, got)
    assert e32 <= REPLAY_TOL


# ================================================================================================ 3. mask sources
@pytest.mark.parametrize("two,row,pad", ROW_ONE_PAD, ids=_id)
def test_mask_sources_agree(ops, two, row, pad):
    """explicit uniforms == the same uniforms bit-packed; the in-kernel Philox draw == ops.philox_uniform fed explicitly (and packed)"""
    r = run(ops, two, row, pad)
    _, _, _, B, H, W = geometry(two, row)
    pu = torch.stack([ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0 + t) for t in range(TN)])
    assert 0.25 < float((pu + RATE).floor().mean()) < 0.75
    with ops.dynca_precision("bf16"):
        packed = history(ops, r, two, pad, ops.pack_fire_mask(r["us"][:TN], RATE, "dynca"))
        fed = history(ops, r, two, pad, pu)
        drawn = history(ops, r, two, pad, None, seed=PHILOX_SEED, step0=PHILOX_STEP0)
        fed_bits = history(ops, r, two, pad, ops.pack_fire_mask(pu, RATE, "dynca"))
    assert same_bits(packed, r["states"]), (row, pad)
    assert same_bits(drawn, fed) and same_bits(fed_bits, fed), (row, pad)
    assert not same_bits(fed, r["states"])                             # other masks than the table's: the comparison is not vacuous


# ================================================================================================ 4. forms agree
@pytest.mark.parametrize("two,row,pad", VEC_ROW_PADS, ids=_id)
def test_unaligned_view_equals_the_aligned_call(ops, two, row, pad):
    """ncahip_dynca_step_fwd_f32 / _ms_f32 on a contiguous view one float into its buffer: x_in & 15 != 0, so launch_dynca_class picks
    the any-shape kernel although W % 4 == 0.  Bit for bit, see the module docstring (4)."""
    from ncahip import _capi
    r = run(ops, two, row, pad)
    C, fc, cc, B, H, W = geometry(two, row)
    w, cond, u, x = r["w"], r["cond"], r["us"][0].contiguous(), r["x"]
    buf = torch.zeros(x.numel() + 8, device=DEV)
    view = buf[1:1 + x.numel()].view_as(x)
    view.copy_(x)
    assert x.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert bf16_form(H, W, x.data_ptr()) == "vec" == (TWO if two else SINGLE)[row][2] and bf16_form(H, W, view.data_ptr()) == "any"
    L, P, pm = ops.lib(), ops._p, ops.PAD_MODES[pad]
    pc = torch.empty(B, 4 * C, H // 2, W // 2, device=DEV) if two else None
    outs = []
    with ops.dynca_precision("bf16"):
        for src in (x, view):
            out = torch.zeros_like(x)
            args = (P(src), P(out), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, pm, RATE, 0, 0)
            if two:
                _capi.check(L.ncahip_dynca_step_fwd_ms_f32(*args, P(pc), ops._stream()), "dynca_step_fwd_ms")
            else:
                _capi.check(L.ncahip_dynca_step_fwd_f32(*args, ops._stream()), "dynca_step_fwd")
            outs.append(out)
    ops.check_errors()
    assert same_bits(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
    assert same_bits(outs[0], r["states"][1])                          # and the first step of the recorded history (held to float64 above)


# ================================================================================================ 5. steered instantiations
@pytest.mark.parametrize("two,row,pad", ROW_ONE_PAD, ids=_id)
def test_identity_field_equals_the_unattached_call(ops, two, row, pad):
    """DyncaSteered<DyncaFwdBf | DyncaFwdMsBf> of the row's class and form with the identity field (s, c) = (0, 1): the bits of the
    unsteered kernel, which section 1 holds to float64; a turned field gives another result"""
    from ncahip import steer
    r = run(ops, two, row, pad)
    _, _, _, _, H, W = geometry(two, row)
    with ops.dynca_precision("bf16"):
        with ops.dynca_direction(steer.direction_field("cartesian", 0.0, H, W, DEV)):
            steered = history(ops, r, two, pad, r["us"][:TN])
        with ops.dynca_direction(steer.direction_field("cartesian", 40.0, H, W, DEV)):
            turned = history(ops, r, two, pad, r["us"][:TN])
    assert same_bits(steered, r["states"]), (row, pad, float((steered - r["states"]).abs().max()))
    if H * W > 1:                                                      # (a plane of one cell has no gradient to turn)
        assert not same_bits(turned, r["states"])                      # the field is honoured at all


# ================================================================================================ 6. persistent kernels
@pytest.mark.parametrize("two,row,pad", PERSIST_ROW_PADS, ids=_id)
def test_persistent_equals_per_step_bit_for_bit(ops, two, row, pad):
    """launch_cfg<MS, CP, FC, HAS_COND, true>: T = 1 and 4, explicit uniforms and in-kernel Philox; the per-step run of the same
    inputs is the history section 1 holds to float64"""
    r = run(ops, two, row, pad)
    C, fc, cc, B, H, W = geometry(two, row)
    x, cond, w = r["x"], r["cond"], r["w"]
    assert ops.lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, cc) > 0
    for T in (1, 4):
        for u_arg in (r["us"][:T], None):
            res = {}
            with ops.dynca_precision("bf16"):
                for persistent in (True, False):
                    ops.persistent_steps = persistent
                    out, states = ops.dynca_nsteps(x, T, cond, u_arg, w, pad, RATE, seed=PHILOX_SEED, step0=3, two_scale=two)
                    assert (states is None) == persistent, "the one-launch kernel did not take the call" if persistent else "unexpected route"
                    res[persistent] = out.clone()
            ops.persistent_steps = False
            assert same_bits(res[True], res[False]), (row, pad, T, u_arg is None, float((res[True] - res[False]).abs().max()))
            f32 = ops.dynca_nsteps(x, T, cond, u_arg, w, pad, RATE, seed=PHILOX_SEED, step0=3, two_scale=two)[0]
            assert not same_bits(f32, res[True])
            if T == 1 and u_arg is not None:
                assert same_bits(res[True], r["states"][1])            # the chain back to float64: the replayed history's first step
    ops.check_errors()


# ================================================================================================ 7. range edge
def test_range_edge(ops):
    assert ops.dynca_bf16_ok(16, 128) and not ops.dynca_bf16_ok(17, 128) and not ops.dynca_bf16_ok(16, 129)
    C, fc, cc, B, H, W = 16, 129, 2, 1, 6, 8
    prm, x, cond, u = bf16_inputs(C, fc, cc, B, H, W, seed=77, device=DEV)
    w = _weights(ops, prm, x)
    res = {}
    for mode in ("f32", "bf16"):
        with ops.dynca_precision(mode):
            res[mode] = ops.dynca_nsteps(x, 1, cond, u[None], w, "replicate", RATE, keep_history=True)[1][1].clone()
    assert same_bits(res["bf16"], res["f32"])                          # fc = 129: the sliced fp32 ladder, whatever the mode
    p64 = {k: v.double() for k, v in prm.items()}
    assert rel_err(res["f32"], O.dynca_step(x.double(), cond.double(), u, p64, "replicate", RATE)) <= REPLAY_TOL
    prm, x, cond, u = bf16_inputs(16, 128, cc, B, H, W, seed=78, device=DEV)      # one hidden unit fewer: the mode applies
    w = _weights(ops, prm, x)
    for mode in ("f32", "bf16"):
        with ops.dynca_precision(mode):
            res[mode] = ops.dynca_nsteps(x, 1, cond, u[None], w, "replicate", RATE, keep_history=True)[1][1].clone()
    assert not same_bits(res["bf16"], res["f32"])


# ================================================================================================ the figures per class
def test_print_the_worst_figures_per_class(ops):
    """what the replays above measured, per instantiation (DESIGN.md quotes this table); asserts nothing the replays did not"""
    print()
    for cls in sorted(_WORST, key=str):
        two, (cp, fcp), has_cond, form = cls
        ratio, frac, at_ratio, at_frac = _WORST[cls]
        print(f"[bf16 ref] {'DyncaFwdMsBf' if two else 'DyncaFwdBf  '} <{cp},{fcp},{str(has_cond).lower()}> {form}: worst |d| / E {ratio:.3f} at {at_ratio}, "
              f"worst cap-(b) fraction {100 * frac:.3f} % at {at_frac} (cap {100 * FLIP_FRACTION:g} %)")
        assert ratio <= 1 + 2.0 ** -7 and frac <= FLIP_FRACTION
