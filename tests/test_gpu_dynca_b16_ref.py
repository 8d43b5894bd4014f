"""The bf16-storage DyNCA step and its backward, held to the documented contract "same kernel, exact f32 compute,
round-to-nearest-even on store" with nothing excluded and no tolerance of its own: the sibling of test_gpu_dynca_ref.py for
ncahip_dynca_step_fwd_bf16 / ncahip_dynca_nsteps_fwd_bf16 (variant DyncaFwdB16 of dynca_step_fwd_kernel: loader pos_load_b16,
store nca_f32_to_b16) and ncahip_dynca_nsteps_bwd_bf16 (widen_bf16_kernel, then the fp32 backward).

Rows: every row of test_gpu_dynca_ref.CASES with fc <= 128, every pad mode it admits, T = 3, rate 0.5, persistent kernel off, the
inputs and uniforms of test_gpu_dynca_ref.make_inputs at that file's seeds.  tests/test_dynca_b16_ref_host.py (ROWS) names the
class and the vector / any-shape form each row reaches and checks the helpers used here on the CPU.

  1  every stored element against float64, teacher-forced: y64 = the oracle's step from the stored state; the stored s must have
     lo(s) - REPLAY_TOL <= y64 <= hi(s) + REPLAY_TOL, lo / hi the midpoints to s's bf16 neighbours.  util.REPLAY_TOL is the
     project's bound for one fp32 step from the same input; no other number enters.  Cells that did not fire keep their bits.
  2  bit for bit against the fp32 kernel: its step from the widened stored state, rounded by torch, equals the stored state.
  3  exact ties: x + b2 with sums on, one step past and just off a rounding boundary, against integer RNE.
  4  forms agree bit for bit: unaligned view (any-shape kernel at W % 4 == 0), ring 2 against ring T + 1, the three mask sources.
  5  backward: all five gradients bit-equal to the fp32 backward of the widened history on every row; the float64 VJP at the stored
     states on a row of class <16,128>; B C H W % 4 != 0 runs forward and is NCAHIP_ERANGE backward.

Every test prints what it measured (-s)."""
import pytest
import torch

from oracle import nca_oracle as O
from test_dynca_b16_ref_host import BF16_VJP_SEEDS, ROWS, TIE_C, TIE_FC, TIE_H, b16_form, bits_of, interval_check, tie_case
from test_gpu_configs import rand_dynca_prm
from test_gpu_dynca_ref import (CASES, GRAD_KEYS, PHILOX_SEED, PHILOX_STEP0, SEEDS, TN, _c64, admits, check_grads, gate_count_at,
                                make_inputs, ops, reference_at_states)      # noqa: F401  (ops: the fixture, persistent kernel off)
from test_gpu_fullsize_ref import DEV, _dyn_w, _f64, _say
from util import REPLAY_TOL

pytestmark = pytest.mark.gpu
ROW_PADS = [(c, p) for c in ROWS for p in O.PAD_MODES if admits(c, p)]
RATE = 0.5

_RUNS = {}


def run(ops, case, pad):
    """inputs, the recorded bf16 history and the float64 step from every stored state of one (row, pad): computed once, shared,
    left unchanged"""
    if (case, pad) not in _RUNS:
        prm, x0, cond, us, cot = make_inputs(case, SEEDS[case, pad])
        p64, w = _f64(prm), _dyn_w(ops, prm, x0)
        _, states = ops.dynca_nsteps(x0.bfloat16(), TN, cond, us, w, pad, RATE, keep_history=True)
        ops.check_errors()
        assert states.dtype == torch.bfloat16 and states.shape == (TN + 1,) + tuple(x0.shape)
        with torch.no_grad():
            y64 = [O.dynca_step(states[t].double(), _c64(cond), us[t], p64, pad, RATE) for t in range(TN)]
        _RUNS[case, pad] = dict(prm=prm, p64=p64, w=w, x0=x0, cond=cond, us=us, cot=cot, states=states, y64=y64)
    return _RUNS[case, pad]


def history(ops, r, pad, us="explicit", **kw):
    us = r["us"] if isinstance(us, str) else us
    return ops.dynca_nsteps(r["x0"].bfloat16(), TN, r["cond"], us, r["w"], pad, RATE, **kw)


# ================================================================================================ 1. rounding intervals against float64
@pytest.mark.parametrize("case,pad", ROW_PADS)
def test_stored_states_lie_in_their_rounding_interval(ops, case, pad):
    r = run(ops, case, pad)
    states, us = r["states"], r["us"]
    worst, flips, kept = 0.0, 0, 0
    for t in range(TN):
        b_in, b_out = bits_of(states[t]), bits_of(states[t + 1])
        assert not bool((b_in == 0x8000).any()), (t, "a -0 among the inputs")
        bad, w, f = interval_check(states[t + 1], r["y64"][t])
        worst, flips = max(worst, w), flips + f
        assert not bool(bad.any()), (case, pad, t, int(bad.sum()), w)
        idle = ((us[t] + RATE).floor() == 0).expand_as(b_in)          # cells that did not fire keep their bits
        kept += int(idle.sum())
        assert torch.equal(b_out[idle], b_in[idle]), (case, pad, t)
    fired = 1.0 - kept / (TN * states[0].numel())
    _say(f"b16 interval {case} {CASES[case]} {pad} {ROWS[case]}", worst_excess_over_replay_tol=worst, bound=1.0, flips=flips,
         elements=TN * states[0].numel(), fired=fired)
    assert 0.2 < fired < 0.8 or states[0][0, 0].numel() < 8            # both kinds of cell are there (tiny planes: whatever they drew)


# ================================================================================================ 2. bit for bit against the fp32 kernel
@pytest.mark.parametrize("case,pad", ROW_PADS)
def test_bit_for_bit_against_the_fp32_kernel(ops, case, pad):
    """the fp32 per-step kernel (pinned to float64 per class by test_gpu_dynca_ref.py) from the widened stored state, rounded by
    torch: the stored state"""
    r = run(ops, case, pad)
    diff = 0
    for t in range(TN):
        _, s32 = ops.dynca_nsteps(r["states"][t].float(), 1, r["cond"], r["us"][t:t + 1], r["w"], pad, RATE, keep_history=True)
        ops.check_errors()
        assert s32.dtype == torch.float32
        d = int((bits_of(s32[1].bfloat16()) != bits_of(r["states"][t + 1])).sum())
        diff += d
        assert torch.equal(s32[1].bfloat16(), r["states"][t + 1]), (case, pad, t, d)
    _say(f"b16 vs fp32 kernel {case} {pad}", differing_elements=diff)


# ================================================================================================ 3. exact ties
@pytest.mark.parametrize("W", [32, 30])
@pytest.mark.parametrize("pad", ["replicate", "circular"])
def test_exact_ties(ops, W, pad):
    """w2 = 0: dx = b2 exactly, rate 1.0 with u = 0: every cell fires.  W = 32 is the vector form, W = 30 the any-shape form"""
    x, b2, want, _ = tie_case(W)
    prm = rand_dynca_prm(TIE_C, TIE_FC, 0, seed=41, scale=3.0)
    prm["w2.weight"] = torch.zeros_like(prm["w2.weight"])
    prm["w2.bias"] = b2.clone()
    xd = x.to(DEV)
    w = _dyn_w(ops, prm, xd)
    u = torch.zeros(1, 1, 1, TIE_H, W, device=DEV)
    got, _ = ops.dynca_nsteps(xd, 1, None, u, w, pad, 1.0)
    ops.check_errors()
    assert got.dtype == torch.bfloat16 and b16_form(W, xd.data_ptr()) == ("vec" if W == 32 else "any")
    miss = int((bits_of(got).cpu() != want).sum())
    _say(f"b16 ties W={W} {pad}", elements=want.numel(), differing=miss)
    assert torch.equal(bits_of(got).cpu(), want), miss


# ================================================================================================ 4. forms agree
@pytest.mark.parametrize("case,pad", [("band", "reflect"), ("band", "constant"), ("c32", "circular"), ("c32", "replicate")])
def test_unaligned_view_equals_the_aligned_call(ops, case, pad):
    """ncahip_dynca_step_fwd_bf16 on a contiguous view one element into its buffer: x_in & 7 != 0, so launch_dynca_class picks the
    any-shape kernel whatever W is (band: W % 4 == 0, the aligned call is the vector form)"""
    from ncahip import _capi
    r = run(ops, case, pad)
    C, fc, cc, B, H, W = CASES[case]
    w, cond, u = r["w"], r["cond"], r["us"][0].contiguous()
    x = r["states"][0].clone()
    buf = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device=DEV)
    view = buf[1:1 + x.numel()].view_as(x)
    view.copy_(x)
    assert x.data_ptr() % 8 == 0 and view.data_ptr() % 8 == 2 and view.is_contiguous()
    assert b16_form(W, x.data_ptr()) == ROWS[case][1] and b16_form(W, view.data_ptr()) == "any"
    L, P, pm = ops.lib(), ops._p, ops.PAD_MODES[pad]
    outs = []
    for src in (x, view):
        out = torch.zeros_like(x)
        _capi.check(L.ncahip_dynca_step_fwd_bf16(P(src), P(out), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc,
                                                 pm, RATE, 0, 0, ops._stream()), "dynca_step_fwd_bf16")
        outs.append(out)
    ops.check_errors()
    assert torch.equal(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
    assert torch.equal(outs[1], r["states"][1])                        # and the first step of the recorded history (held to float64 above)


@pytest.mark.parametrize("case,pad", [("rem16v", "reflect"), ("rem16v", "circular"), ("c20", "constant"), ("c20", "replicate")])
def test_ring_of_two_equals_the_kept_history(ops, case, pad):
    r = run(ops, case, pad)
    last, ring = history(ops, r, pad)
    ops.check_errors()
    assert ring.shape[0] == 2 and last.dtype == torch.bfloat16
    assert torch.equal(last, r["states"][TN])
    assert torch.equal(ring[(TN - 1) % 2], r["states"][TN - 1])


@pytest.mark.parametrize("case,pad", [("rem12", "constant"), ("rem12", "reflect"), ("cond4", "circular"), ("cond4", "replicate")])
def test_mask_sources_agree(ops, case, pad):
    """explicit uniforms == the same uniforms bit-packed; the in-kernel Philox draw == philox_uniform fed explicitly (and packed)"""
    r = run(ops, case, pad)
    C, fc, cc, B, H, W = CASES[case]
    bits = ops.pack_fire_mask(r["us"], RATE, "dynca")
    _, packed = history(ops, r, pad, bits, keep_history=True)
    assert torch.equal(packed, r["states"])
    pu = torch.stack([ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0 + t) for t in range(TN)])
    for t in range(TN):
        assert (pu[t].cpu().numpy() == O.philox_uniform(PHILOX_SEED, PHILOX_STEP0 + t, B, H, W)).all(), t
    assert 0.2 < float((pu + RATE).floor().mean()) < 0.8
    _, fed = history(ops, r, pad, pu, keep_history=True)
    _, drawn = history(ops, r, pad, None, keep_history=True, seed=PHILOX_SEED, step0=PHILOX_STEP0)
    _, fed_bits = history(ops, r, pad, ops.pack_fire_mask(pu, RATE, "dynca"), keep_history=True)
    ops.check_errors()
    assert torch.equal(drawn, fed) and torch.equal(fed_bits, fed)
    assert not torch.equal(fed, r["states"])                           # other masks than the table's: the comparison is not vacuous


# ================================================================================================ 5. backward
@pytest.mark.parametrize("case,pad", ROW_PADS)
def test_backward_equals_the_fp32_backward_of_the_widened_history(ops, case, pad):
    """ncahip_dynca_nsteps_bwd_bf16 is a storage format: all five gradients bit-equal to ncahip_dynca_nsteps_bwd_f32 on states.float()"""
    r = run(ops, case, pad)
    g16 = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], r["w"], r["cot"], None, TN, pad, RATE)
    g16 = {k: v.clone() for k, v in g16.items()}
    g32 = ops.dynca_nsteps_backward(r["states"].float(), r["cond"], r["us"], r["w"], r["cot"], None, TN, pad, RATE)
    ops.check_errors()
    assert set(g16) == set(GRAD_KEYS)
    for k in GRAD_KEYS:
        assert g16[k].dtype == torch.float32 and bool(torch.isfinite(g16[k]).all()), k
        assert torch.equal(g16[k], g32[k]), (case, pad, k, int((g16[k] != g32[k]).sum()))
    assert float(g16["w1"].abs().max()) > 0 and float(g16["x0"].abs().max()) > 0


@pytest.mark.parametrize("case,pad", list(BF16_VJP_SEEDS))
def test_backward_against_the_float64_vjp_at_the_stored_states(ops, case, pad):
    """as test_gpu_dynca_ref.test_bf16_history_backward, on a row of class <16,128>: the chain of per-step float64 VJPs at the states
    the device stored, zero gates counted on those same states; the seed keeps them 4 x DYNCA_GATE_K away on the CPU's emulation"""
    prm, x0, cond, us, cot = make_inputs(case, BF16_VJP_SEEDS[case, pad])
    p64, w = _f64(prm), _dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0.bfloat16(), TN, cond, us, w, pad, RATE, keep_history=True)
    g = ops.dynca_nsteps_backward(states, cond, us, w, cot, None, TN, pad, RATE)
    ops.check_errors()
    gates = gate_count_at(p64, states, cond, us, pad, RATE)
    worst, flips = 0.0, 0
    with torch.no_grad():
        for t in range(TN):
            y64 = O.dynca_step(states[t].double(), _c64(cond), us[t], p64, pad, RATE)
            bad, wt, f = interval_check(states[t + 1], y64)
            assert not bool(bad.any()), t
            worst, flips = max(worst, wt), flips + f
    print(f"\n[ref] b16 float64 vjp {case} {pad}: gates on the stored states {gates}, flips {flips}, worst excess / REPLAY_TOL {worst:.3e}")
    assert gates == 0, "a gate on the device's stored states: pick another seed (python tests/test_dynca_b16_ref_host.py)"
    check_grads(f"b16 float64 vjp {case} {pad}", g, reference_at_states(p64, states, cond, us, pad, RATE, cot))


def test_backward_refuses_a_history_that_is_no_multiple_of_four(ops):
    """1 x 5 x 3 x 3: the forward runs (any-shape form, held to the interval criterion), widen_bf16_kernel's four-element groups do not
    cover 45 elements and the backward says NCAHIP_ERANGE before it enqueues anything"""
    from ncahip import _capi
    B, C, H, W, fc = 1, 5, 3, 3, 24
    prm = rand_dynca_prm(C, fc, 0, seed=43, scale=3.0)
    gen = torch.Generator().manual_seed(44)
    x0 = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    us = torch.rand(TN, B, 1, H, W, generator=gen).to(DEV)
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    w = _dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0.bfloat16(), TN, None, us, w, "replicate", RATE, keep_history=True)
    ops.check_errors()
    p64 = _f64(prm)
    with torch.no_grad():
        for t in range(TN):
            bad, worst, _ = interval_check(states[t + 1], O.dynca_step(states[t].double(), None, us[t], p64, "replicate", RATE))
            assert not bool(bad.any()), (t, worst)
    with pytest.raises(_capi.NcaHipError, match=rf"rc={_capi.ERANGE}\)"):
        ops.dynca_nsteps_backward(states, None, us, w, cot, None, TN, "replicate", RATE)
    g = ops.dynca_nsteps_backward(states.float(), None, us, w, cot, None, TN, "replicate", RATE)      # the fp32 history of the same shape is served
    ops.check_errors()
    assert bool(torch.isfinite(g["x0"]).all())
