"""Full-size kernel paths against a float64 reference on the device.

The CPU oracle needs minutes at the sizes the project ships, so the large tests elsewhere compare kernel families with each other
(tile == generic), use periodicity, or check properties (linearity, determinism).  None of those sees a bug both families share
(a helper, a Philox counter, an offset), a pad-mode border, or a wrong but linear and deterministic backward.  Here the reference
is the oracle itself (oracle/nca_oracle.py) run in float64 on the GPU with the same uniforms; tests/test_oracle_float64.py pins
that mode to the reference-generated fp32 fixtures.

Bounds are the small-shape ones: REL_TOL forward (cells whose pooled alpha lies within 2e-6 of the life threshold excluded), 2e-4
max-norm for per-cell gradients outside the influence region of ReLU gates the float64 trajectory itself puts within rounding
of zero (nca_oracle.*_gate_influence), 2e-4 of the largest entry for weight gradients; bf16 storage at the budgets of
tests/test_gpu_bf16.py.  Each family also runs a negative control: the same comparison against the reference evaluated with
ONE parameter entry changed by a relative 1e-3 must miss its bound.

Every test prints its measured errors next to the bounds, the exclusions, its wall time and its peak device memory (-s)."""
import gc
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_gpu_configs import rand_cond_prm, rand_dynca_prm
from util import GATE_K, REL_TOL, grads_match_outside

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ULP = 2.0 ** -8
NEAR = 2e-6          # pooled alpha this close to the life threshold may resolve either way between fp32 and float64
GTOL = 2e-4          # per-cell gradients (outside the gate-influence region) and weight gradients
DYNCA_GATE_K = 4e-6  # relative gate margin for the 67..131-term DyNCA hidden layer (test_gpu_parity._dynca_gate_ambiguous)
PERTURB = 1e-3       # negative controls: one parameter entry scaled by 1 + PERTURB
COND_NAMES = {"wp": "perception_net.weight", "w1": "update_net.out.0.weight", "b1": "update_net.out.0.bias",
              "w2": "update_net.out.2.weight", "b2": "update_net.out.2.bias", "w3": "update_net.out.4.weight"}
DYNCA_NAMES = {"w1": "w1.weight", "b1": "w1.bias", "w2": "w2.weight", "b2": "w2.bias"}


@pytest.fixture(scope="module")
def ops():
    with gpu_ops() as o:
        yield o


@pytest.fixture(autouse=True)
def _cost(request):
    """wall time and peak device memory of every test; large tensors are freed between tests"""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[cost] {request.node.name}: {time.time() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def _say(case, **kv):
    print(f"\n[ref] {case}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _f64(prm):
    return {k: v.to(DEV, F64) for k, v in prm.items()}


def _cond_w(ops, prm, like):
    return ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                           prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], like)


def _dyn_w(ops, prm, like):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], like)


def _rel(got, ref, keep=None):
    """max |got - ref| / max(1, max |ref|) (util.rel_err) over the cells `keep` [B,1,H,W] (all when None), on the device"""
    got, ref = got.detach().double(), ref.detach().double()
    scale = max(1.0, float(ref.abs().max()))
    d = (got - ref).abs()
    if keep is not None:
        d = d[keep.expand_as(d)]
    return float(d.max()) / scale if d.numel() else 0.0


def _rmax(got, ref):
    """max |got - ref| / max |ref|: gradients"""
    got, ref = got.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-12)


def _rel2(got, ref):
    got, ref = got.detach().double().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-12))


def _near(x, alive=3, thr=0.1, eps=NEAR):
    """[B,1,H,W]: cells whose 3x3-pooled alpha lies within eps of the threshold"""
    return (F.max_pool2d(x[:, alive:alive + 1].double(), 3, 1, 1) - thr).abs() < eps


def _dilate(m, r, circular=False):
    if r <= 0:
        return m
    if circular:
        return F.max_pool2d(F.pad(m.float(), (r, r, r, r), mode="circular"), 2 * r + 1, 1, 0) > 0
    return F.max_pool2d(m.float(), 2 * r + 1, 1, r) > 0


def _perturbed(prm, key, idx):
    p = {k: v.clone() for k, v in prm.items()}
    p[key].view(-1)[idx] *= 1.0 + PERTURB
    return p


def _lever_entry(w, h):
    """flat index of the output-layer entry (w [O,K,1,1], input activations h [B,K,H,W]) with the largest |w_ok| * max|h_k|:
    the single weight whose perturbation moves the output most"""
    hk = h.detach().abs().amax(dim=(0, 2, 3)).to(w.device, w.dtype)
    return int((w.reshape(w.shape[0], -1).abs() * hk[None, :]).argmax())


def _cond_hidden2(p, prm):
    h1 = F.relu(O._conv1x1(p, prm["update_net.out.0.weight"], prm["update_net.out.0.bias"]))
    return F.relu(O._conv1x1(h1, prm["update_net.out.2.weight"], prm["update_net.out.2.bias"]))


def _cond_inputs(B, C, gch, S, Tn, seed, straddle):
    """x (alpha of the first half of the batch scaled into [0, 0.12): life masks straddle the threshold), goal, us, cot"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, S, S, generator=gen)
    if straddle:
        x[: B // 2, 3] *= 0.12
    goal = torch.randn(B, gch, S, S, generator=gen) * 0.5
    us = torch.rand(Tn, B, 1, S, S, generator=gen)
    cot = torch.randn(B, C, S, S, generator=gen)
    return x.to(DEV), goal.to(DEV), us.to(DEV), cot.to(DEV)


# ================================================================================================ ConditionedNCA, fp32
def _cond_forward_fp32(ops, case, prm, x, goal, us, control=False):
    """teacher-forced single steps (ncahip_cond_step_fwd + finalize) and the free-running grow loop, tile and generic kernels"""
    B, C, H, W = x.shape
    Tn = us.shape[0]
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.double(), C)
    ins, refs, nears = [], [], []
    xi = x
    with torch.no_grad():
        for t in range(Tn):
            d = O.cond_step(xi.double(), gpad, us[t], p64, 3, return_all=True)
            ins.append(xi)
            refs.append(d["x2"])
            nears.append(_near(xi) | _near(d["x1"]))
            if t == 0 and control:
                key, idx = "update_net.out.4.weight", _lever_entry(p64["update_net.out.4.weight"], _cond_hidden2(d["p"], p64))
            xi = d["x2"].float()
            del d
        # free-running float64; a life flip at step t moves the state within Chebyshev distance 2 per later step
        xr, amb = x.double(), torch.zeros_like(nears[0])
        for t in range(Tn):
            d = O.cond_step(xr, gpad, us[t], p64, 3, return_all=True)
            amb |= _near(xr) | _near(d["x1"])
            xr = d["x2"]
            del d
    region = _dilate(amb, 2 * Tn)
    excl = sum(int(n.sum()) for n in nears)
    assert excl < 1e-3 * B * H * W * Tn, excl            # the exclusion is a handful of cells, not a loophole
    assert float(region.float().mean()) < 1e-2
    w = _cond_w(ops, prm, x)
    worst_tf, worst_free = 0.0, 0.0
    for variant in (0, 1):
        ops.force_generic(variant)
        try:
            for t in range(Tn):
                xp, pre = ops.cond_step(ins[t], None, goal, us[t], w, 3)
                x2 = ops.cond_finalize(xp, pre, 3)
                worst_tf = max(worst_tf, _rel(x2, refs[t], ~nears[t]))
                del xp, pre, x2
            out, _, _ = ops.cond_grow(x, Tn, goal, us, w, 3)
            worst_free = max(worst_free, _rel(out, xr, ~region))
            if variant == 0:
                last = out.clone()
            del out
        finally:
            ops.force_generic(0)
    ops.check_errors()
    alive = float(O.cond_alive(xr, 3).float().mean())
    _say(case + " fwd", teacher_forced=worst_tf, free_running=worst_free, bound=REL_TOL, near_cells_excluded=excl,
         free_running_cells_excluded=int(region.sum()), alive_fraction=alive)
    assert worst_tf < REL_TOL and worst_free < REL_TOL, (worst_tf, worst_free)
    if control:
        # one step moves the state by at most 1e-3 |w_ij h_j| ~ REL_TOL: the free-running grow loop accumulates it over Tn steps
        with torch.no_grad():
            bad = O.cond_grow(x.double(), gpad, list(us), _f64(_perturbed(prm, key, idx)), 3)
        e = _rel(last, bad, ~region)
        _say(case + " fwd negative control", entry=f"{key}[{idx}]", err=e, bound=REL_TOL)
        assert e > REL_TOL, e


def _cond_backward_fp32(ops, case, prm, x0, goal, us, cot, control=False):
    """dL/dx0 and dL/dgoal outside the gate-influence region with the full cotangent; then every gradient -- dL/dx0 and dL/dgoal
    at every cell, the six weight gradients -- with the cotangent zeroed where an ambiguous gate could see it (_quiet_cot)"""
    B, C, H, W = x0.shape
    gch, Tn = goal.shape[1], us.shape[0]
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.double(), C)
    with torch.no_grad():          # precondition: no life mask of the float64 trajectory anywhere near its threshold
        xr, margin = x0.double(), float("inf")
        for t in range(Tn):
            d = O.cond_step(xr, gpad, us[t], p64, 3, return_all=True)
            for s in (xr, d["x1"]):
                margin = min(margin, float((F.max_pool2d(s[:, 3:4], 3, 1, 1) - 0.1).abs().min()))
            xr = d["x2"]
            del d
        del xr
    assert margin > 1e-3, margin
    w = _cond_w(ops, prm, x0)
    out, states, pre = ops.cond_grow(x0, Tn, goal, us, w, 3, keep_history=True)
    gr = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, 3)
    _, gx, gg, gw = O.cond_grow_loss_grads(x0.double(), gpad, list(us), p64, 3, 0.1, 0.5, cot.double())
    gg = gg[:, C - gch:]
    region, cnt = O.cond_gate_influence(x0.double(), gpad, list(us), p64, 3, GATE_K)
    ok1, out1, in1 = grads_match_outside(gr["x0"], gx, region.cpu(), GTOL)
    ok2, out2, in2 = grads_match_outside(gr["goal"], gg, region.cpu(), GTOL)
    ex, eg = _err_outside(gr["x0"], gx, region), _err_outside(gr["goal"], gg, region)
    full = {k: (_rmax(gr[k], gw[n]), _rel2(gr[k], gw[n])) for k, n in COND_NAMES.items()}
    del gx, gg, gw
    cq, quiet = _quiet_cot(cot, region, Tn)
    gq = ops.cond_grow_backward(states, pre, goal, us, w, cq, Tn, 3)
    ops.check_errors()
    del out, states, pre, gr
    ref = O.cond_grow_loss_grads(x0.double(), gpad, list(us), p64, 3, 0.1, 0.5, cq.double())
    eq = _cond_grad_errs(gq, ref, C, gch)
    _say(case + " bwd", x0_outside_region=ex, goal_outside_region=eg, bound=GTOL, gates_excluded=int(cnt.sum()),
         cells_excluded=int(region.sum()), x0_misses_inside=in1, goal_misses_inside=in2,
         full_cot_weights_max=max(v[0] for v in full.values()), full_cot_weights_l2=max(v[1] for v in full.values()),
         quiet_cot_cells_zeroed=int((~quiet).sum()), **{f"quiet_{k}": v for k, v in eq.items()})
    assert cnt.sum() == 0 or region.any()
    assert ok1 and ok2, (out1, in1, out2, in2)
    for k, e in eq.items():
        assert e < GTOL, (k, e)
    for k, (emax, el2) in full.items():      # full cotangent: the weight-gradient bound of test_cfg3_..._on_crops for excused gates
        assert el2 < 1e-3 and emax < 1e-2, (k, emax, el2)
    if control:
        worst, which = _control(lambda q: _cond_grad_errs(gq, O.cond_grow_loss_grads(x0.double(), gpad, list(us), _f64(q), 3, 0.1, 0.5,
                                                                                      cq.double()), C, gch),
                                prm, list(COND_NAMES.values()))
        _say(case + " bwd negative control", entry=which, err=worst, bound=GTOL)
        assert worst > GTOL, worst


def _cond_grad_errs(g, ref, C, gch):
    _, gx, gg, gw = ref
    e = {"x0": _rmax(g["x0"], gx), "goal": _rmax(g["goal"], gg[:, C - gch:])}
    e.update({k: _rmax(g[k], gw[n]) for k, n in COND_NAMES.items()})
    return e


def _quiet_cot(cot, region, Tn, circular=False):
    """The cotangent with every cell zeroed from which the adjoint can reach an ambiguous ReLU gate.  `region` holds the cells
    within Chebyshev distance t + 1 of a gate at step t whose relative margin on the float64 trajectory is below the gate bound;
    the adjoint of x_{t+1} at a cell depends on the cotangent within distance Tn - 1 - t, so zeroing `region` grown by Tn leaves
    every ambiguous gate with an exactly zero adjoint: however such a gate resolves, no gradient moves (its forward effect is of
    the order of its margin).  The strict bounds then hold everywhere with nothing excluded."""
    quiet = ~_dilate(region, Tn, circular)
    return cot * quiet, quiet


def _control(errs_for, prm, keys):
    """Negative control: among the largest-|w| entry of each weight tensor, the one whose relative 1e-3 change the comparison
    sees most; returns (worst error against the reference with that entry changed, 'key[index]')"""
    best = (-1.0, None)
    for key in keys:
        if prm[key].dim() < 2:
            continue
        idx = int(prm[key].abs().argmax())
        e = max(errs_for(_perturbed(prm, key, idx)).values())
        best = max(best, (e, f"{key}[{idx}]"))
    return best


def _err_outside(got, ref, region):
    """max |got - ref| / max |ref| over the cells outside `region` [B,1,H,W]"""
    got, ref = got.detach().double(), ref.detach().double()
    d = (got - ref).abs()[~region.expand_as(got)]
    return float(d.max()) / max(float(ref.abs().max()), 1e-6) if d.numel() else 0.0


# ================================================================================================ ConditionedNCA, bf16 storage
def _cond_forward_bf16(ops, case, prm, x, goal, us):
    """teacher-forced bf16 steps against the float64 bf16-faithful step (2 ulp), and the free-running grow loop at the
    small-shape drift budget"""
    B, C, H, W = x.shape
    Tn = us.shape[0]
    p64 = _f64(prm)
    x, goal = x.bfloat16(), goal.bfloat16()
    gpad = O.cond_pad_goal(goal.double(), C)
    w = _cond_w(ops, prm, x)
    worst_p, worst_r, frac, excl = 0.0, 0.0, 0.0, 0
    xi = x
    for t in range(Tn):
        with torch.no_grad():
            ref_next, ref_pre, ref_pend = O.cond_step_bf16(xi.double(), gpad, us[t], p64)
        xp, pre = ops.cond_step(xi, None, goal, us[t], w, 3)
        assert torch.equal(pre.bool().reshape(B, 1, H, W), ref_pre), t
        got = xp.double()
        worst_p = max(worst_p, float(((got - ref_pend).abs() / ref_pend.abs().clamp_min(1.0)).max()))
        frac = max(frac, float((got != ref_pend).float().mean()))
        res = ops.cond_finalize(xp, pre, 3).double()
        unsafe = (F.max_pool2d(ref_pend[:, 3:4], 3, 1, 1) - 0.1).abs() <= 2 * ULP
        excl += int(unsafe.sum())
        worst_r = max(worst_r, float(((res - ref_next).abs() / ref_next.abs().clamp_min(1.0))[~unsafe.expand_as(res)].max()))
        xi = ref_next.bfloat16()
        del xp, pre, res, got, ref_next, ref_pend
    with torch.no_grad():
        ref = x.double()
        for t in range(Tn):
            ref = O.cond_step_bf16(ref, gpad, us[t], p64)[0]
    out, _, _ = ops.cond_grow(x, Tn, goal, us, w, 3)
    err = (out.double() - ref).abs() / ref.abs().clamp_min(1.0)
    drift, mean = float((err > 8 * ULP).float().mean()), float(err.mean())
    ops.check_errors()
    _say(case + " bf16 fwd", pending=worst_p, resolved=worst_r, bound=2 * ULP, differing_fraction=frac,
         resolved_cells_excluded=excl, free_running_over_8ulp=drift, free_running_mean=mean)
    assert worst_p <= 2 * ULP and worst_r <= 2 * ULP and frac < 0.03
    assert drift < 0.01 and mean < 2e-3


def _cond_backward_bf16(ops, case, prm, x0, goal, us, cot):
    B, C, H, W = x0.shape
    gch, Tn = goal.shape[1], us.shape[0]
    p64 = _f64(prm)
    x0, goal = x0.bfloat16(), goal.bfloat16()
    gpad = O.cond_pad_goal(goal.double(), C)
    w = _cond_w(ops, prm, x0)
    out, states, pre = ops.cond_grow(x0, Tn, goal, us, w, 3, keep_history=True)
    g16 = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, 3)
    ops.check_errors()
    del out, states, pre
    tol = 2e-2 if Tn <= 2 else 4e-2
    _, gx, gg, gw = O.cond_grow_bf16_loss_grads(x0.double(), gpad, list(us), p64, 3, 0.1, 0.5, cot.double())
    e_faithful = {"x0": _rel2(g16["x0"], gx), "goal": _rel2(g16["goal"], gg[:, C - gch:])}
    e_faithful.update({k: _rel2(g16[k], gw[n]) for k, n in COND_NAMES.items()})
    del gx, gg, gw
    _, gx, gg, gw = O.cond_grow_loss_grads(x0.double(), gpad, list(us), p64, 3, 0.1, 0.5, cot.double())
    e_fp32 = {"x0": _rel2(g16["x0"], gx), "goal": _rel2(g16["goal"], gg[:, C - gch:])}
    e_fp32.update({k: _rel2(g16[k], gw[n]) for k, n in COND_NAMES.items()})
    _say(case + " bf16 bwd", vs_bf16_faithful=max(e_faithful.values()), bound_faithful=tol, vs_fp32_steps=max(e_fp32.values()),
         bound_fp32=8e-2)
    for k, e in e_faithful.items():
        assert e < tol, (k, e)
    for k, e in e_fp32.items():
        assert e < 8e-2, (k, e)


# default model: C = 20 (3 rgb + alpha + 16 goal channels), hidden 64, 8 x 20 x 256^2, 3 steps
def test_default_model_c20_fp32_vs_float64(ops):
    prm = rand_cond_prm(20, seed=31, out_scale=0.5)
    x, goal, us, _ = _cond_inputs(8, 20, 16, 256, 3, seed=310, straddle=True)
    _cond_forward_fp32(ops, "default C=20 8x256^2", prm, x, goal, us, control=True)
    del x
    x0, goal, us, cot = _cond_inputs(8, 20, 16, 256, 3, seed=311, straddle=False)
    _cond_backward_fp32(ops, "default C=20 8x256^2", prm, x0, goal, us, cot, control=True)


def test_default_model_c20_bf16_vs_float64(ops):
    prm = rand_cond_prm(20, seed=32, out_scale=0.5)
    x, goal, us, _ = _cond_inputs(8, 20, 16, 256, 3, seed=320, straddle=True)
    _cond_forward_bf16(ops, "default C=20 8x256^2", prm, x, goal, us)
    del x
    x0, goal, us, cot = _cond_inputs(8, 20, 16, 256, 3, seed=321, straddle=False)
    _cond_backward_bf16(ops, "default C=20 8x256^2", prm, x0, goal, us, cot)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_cfg3_fully_alive_vs_float64(ops, storage):
    """BASELINE configs[2]'s shape, B = 32 C = 16 256^2, fully alive (the crop test covers mostly dead grids)."""
    prm = rand_cond_prm(16, seed=33, out_scale=0.5)
    x, goal, us, _ = _cond_inputs(32, 16, 12, 256, 3, seed=330, straddle=True)
    (_cond_forward_fp32 if storage == "f32" else _cond_forward_bf16)(ops, "configs[2] 32x16x256^2", prm, x, goal, us)
    del x
    x0, goal, us, cot = _cond_inputs(32, 16, 12, 256, 3, seed=331, straddle=False)
    (_cond_backward_fp32 if storage == "f32" else _cond_backward_bf16)(ops, "configs[2] 32x16x256^2", prm, x0, goal, us, cot)


def test_large_plane_2048_cond_vs_float64(ops):
    """1 x 16 x 2048^2, 2 steps: forward (both kernel families) and backward"""
    prm = rand_cond_prm(16, seed=34, out_scale=0.5)
    x, goal, us, _ = _cond_inputs(2, 16, 12, 2048, 2, seed=340, straddle=True)
    _cond_forward_fp32(ops, "cond 1x16x2048^2 (straddling)", prm, x[:1].contiguous(), goal[:1].contiguous(), us[:, :1].contiguous())
    del x, goal, us
    x0, goal, us, cot = _cond_inputs(1, 16, 12, 2048, 2, seed=341, straddle=False)
    _cond_forward_fp32(ops, "cond 1x16x2048^2", prm, x0, goal, us)
    _cond_backward_fp32(ops, "cond 1x16x2048^2", prm, x0, goal, us, cot)


def test_cond_plane_1024x4096_philox_vs_float64(ops):
    """1 x 12 x 1024 x 4096 (plane bytes above 2^24), 2 steps with the in-kernel Philox mask, both kernel families"""
    B, C, H, W, Tn, seed = 1, 12, 1024, 4096, 2, 7
    prm = rand_cond_prm(C, seed=9, out_scale=2.0)
    gen = torch.Generator().manual_seed(35)
    x = torch.rand(B, C, H, W, generator=gen)
    x[:, 3] *= 0.12
    x = x.to(DEV)
    goal = (torch.randn(B, 8, H, W, generator=gen) * 0.5).to(DEV)
    us = torch.stack([ops.philox_uniform(B, H, W, seed, t) for t in range(Tn)])
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.double(), C)
    with torch.no_grad():
        xr, amb = x.double(), torch.zeros(B, 1, H, W, dtype=torch.bool, device=DEV)
        for t in range(Tn):
            d = O.cond_step(xr, gpad, us[t], p64, 3, return_all=True)
            amb |= _near(xr) | _near(d["x1"])
            xr = d["x2"]
            del d
    region = _dilate(amb, 2 * Tn)
    w = _cond_w(ops, prm, x)
    errs = []
    for variant in (0, 1):
        ops.force_generic(variant)
        try:
            out, _, _ = ops.cond_grow(x, Tn, goal, None, w, 3, seed=seed)
            errs.append(_rel(out, xr, ~region))
            del out
        finally:
            ops.force_generic(0)
    ops.check_errors()
    _say("cond 1x12x1024x4096 philox fwd", tile=errs[0], generic=errs[1], bound=REL_TOL, cells_excluded=int(region.sum()))
    assert float(region.float().mean()) < 1e-2
    assert max(errs) < REL_TOL, errs


# ================================================================================================ DyNCA
def _dynca_case(ops, case, prm, x0, cond, us, cot, pad, control=False, scales_two=False):
    """free-running forward (every state, both kernel families) and dynca_nsteps_backward against float64 autograd; scales_two:
    perception_scales = [0, 1] (the two-scale kernels against the oracle with scales=(0, 1))"""
    sc = (0, 1) if scales_two else (0,)
    Tn = us.shape[0]
    p64 = _f64(prm)
    c64 = cond.double()
    w = _dyn_w(ops, prm, x0)
    with torch.no_grad():
        refs = O.dynca_nsteps(x0.double(), c64, list(us), p64, pad, 0.5, scales=sc, collect=True)[1]
    worst = 0.0
    for variant in (0, 1):
        ops.force_generic(variant)
        try:
            out, states = ops.dynca_nsteps(x0, Tn, cond, us, w, pad, 0.5, keep_history=True, two_scale=scales_two)
            for t in range(Tn):
                worst = max(worst, _rel(states[t + 1], refs[t]))
            if variant == 0:
                hist, last = states, states[Tn].clone()
            else:
                del states
            del out
        finally:
            ops.force_generic(0)
    gr = ops.dynca_nsteps_backward(hist, cond, us, w, cot, None, Tn, pad, 0.5, two_scale=scales_two)
    ops.check_errors()
    _say(case + " fwd", err=worst, bound=REL_TOL)
    assert worst < REL_TOL, worst
    if control:
        key = "w2.weight"
        with torch.no_grad():
            x1 = O.dynca_step(x0.double(), c64, us[0], p64, pad, 0.5, sc, return_all=True)
            h = F.relu(O._conv1x1(x1["y"], p64["w1.weight"], p64["w1.bias"]))
            idx = _lever_entry(p64[key], h)
            del x1, h
            bad = O.dynca_nsteps(x0.double(), c64, list(us), _f64(_perturbed(prm, key, idx)), pad, 0.5, scales=sc)
        e = _rel(last, bad)
        _say(case + " fwd negative control", entry=f"{key}[{idx}]", err=e, bound=REL_TOL)
        assert e > REL_TOL, e
        del bad
    del refs
    _, gx, gw = O.dynca_nsteps_loss_grads(x0.double(), c64, list(us), p64, pad, 0.5, cot.double(), scales=sc)
    region, cnt = O.dynca_gate_influence(x0.double(), c64, list(us), p64, pad, DYNCA_GATE_K, scales=sc)
    ok, nout, nin = grads_match_outside(gr["x0"], gx, region.cpu(), GTOL)
    ex = _err_outside(gr["x0"], gx, region)
    full = {k: (_rmax(gr[k], gw[n]), _rel2(gr[k], gw[n])) for k, n in DYNCA_NAMES.items()}
    del gx, gw, gr
    cq, quiet = _quiet_cot(cot, region, Tn, pad == "circular")
    gq = ops.dynca_nsteps_backward(hist, cond, us, w, cq, None, Tn, pad, 0.5, two_scale=scales_two)
    ops.check_errors()
    del hist
    eq = _dynca_grad_errs(gq, O.dynca_nsteps_loss_grads(x0.double(), c64, list(us), p64, pad, 0.5, cq.double(), scales=sc))
    _say(case + " bwd", x0_outside_region=ex, bound=GTOL, gates_excluded=int(cnt.sum()), cells_excluded=int(region.sum()),
         x0_misses_inside=nin, full_cot_weights_max=max(v[0] for v in full.values()),
         full_cot_weights_l2=max(v[1] for v in full.values()), quiet_cot_cells_zeroed=int((~quiet).sum()),
         **{f"quiet_{k}": v for k, v in eq.items()})
    assert ok, (nout, nin)
    for k, e in eq.items():
        assert e < GTOL, (k, e)
    for k, (emax, el2) in full.items():
        assert el2 < 1e-3 and emax < 1e-2, (k, emax, el2)
    if control:
        worst, which = _control(lambda q: _dynca_grad_errs(gq, O.dynca_nsteps_loss_grads(x0.double(), c64, list(us), _f64(q), pad, 0.5,
                                                                                         cq.double(), scales=sc)),
                                prm, list(DYNCA_NAMES.values()))
        _say(case + " bwd negative control", entry=which, err=worst, bound=GTOL)
        assert worst > GTOL, worst


def _dynca_grad_errs(g, ref):
    _, gx, gw = ref
    e = {"x0": _rmax(g["x0"], gx)}
    e.update({k: _rmax(g[k], gw[n]) for k, n in DYNCA_NAMES.items()})
    return e


def _dynca_inputs(B, C, cc, H, W, Tn, seed):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen) * 2 - 1
    us = torch.rand(Tn, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    return x0.to(DEV), cond.to(DEV), us.to(DEV), cot.to(DEV)


@pytest.mark.parametrize("pad", O.PAD_MODES)
def test_cfg5_dynca_c32_fc256_512_vs_float64(ops, pad):
    """BASELINE configs[4]: DyNCA C = 32, fc = 256 (two 128-wide hidden slices), 3 conditioning channels, 2 x 512^2, 3 steps,
    every pad mode (the periodicity test covers circular only)"""
    prm = rand_dynca_prm(32, 256, 3, seed=41)
    x0, cond, us, cot = _dynca_inputs(2, 32, 3, 512, 512, 3, seed=410 + O.PAD_MODES.index(pad))
    _dynca_case(ops, f"configs[4] DyNCA 2x32x512^2 {pad}", prm, x0, cond, us, cot, pad, control=(pad == "replicate"))


@pytest.mark.parametrize("pad", ["replicate", "reflect", "constant"])
def test_large_plane_2048_dynca_vs_float64(ops, pad):
    """1 x 16 x 2048^2, fc = 128, 2 steps: the pad modes the periodicity test cannot reach"""
    prm = rand_dynca_prm(16, 128, 3, seed=42)
    x0, cond, us, cot = _dynca_inputs(1, 16, 3, 2048, 2048, 2, seed=420 + O.PAD_MODES.index(pad))
    _dynca_case(ops, f"DyNCA 1x16x2048^2 {pad}", prm, x0, cond, us, cot, pad)


# ================================================================================================ persistent B = 1 kernel
@pytest.mark.parametrize("C,fc,two,pad", [(12, 96, False, "replicate"), (12, 96, True, "circular"),
                                          (16, 128, False, "reflect"), (16, 128, True, "constant")])
def test_persistent_largest_frame_vs_float64(ops, C, fc, two, pad):
    """ncahip_dynca_nsteps_fwd_persist{,_ms}_f32 called directly (no silent fall-back to the per-step kernels) at the largest
    frame it accepts on this device, 32 steps, against the float64 reference"""
    from ncahip import _capi
    cc, Tn, rate = 3, 32, 0.5
    prm = rand_dynca_prm(C, fc, cc, seed=43 + C, scale=1.0)
    L = ops.lib()
    ran = None
    for S in (512, 480, 448, 416, 384, 352, 320, 288, 256):
        x0, cond, us, _ = _dynca_inputs(1, C, cc, S, S, Tn, seed=430 + S)
        w = _dyn_w(ops, prm, x0)
        nbytes = L.ncahip_dynca_nsteps_persist_workspace(1, C, S, S, fc, cc)
        if not nbytes:
            continue
        ws, epoch = ops._persist_workspace(nbytes, x0.device)
        out = torch.empty_like(x0)
        fn = L.ncahip_dynca_nsteps_fwd_persist_ms_f32 if two else L.ncahip_dynca_nsteps_fwd_persist_f32
        rc = fn(ops._p(x0), ops._p(out), Tn, ops._p(cond), ops._p(us), ops._p(w.w1), ops._p(w.b1), ops._p(w.w2), ops._p(w.b2), 1, C,
                S, S, fc, cc, ops.PAD_MODES[pad], rate, 0, 0, ops._p(ws), nbytes, epoch, ops._stream())
        if rc == _capi.ERANGE:
            continue
        _capi.check(rc, "dynca_nsteps_fwd_persist")
        torch.cuda.synchronize()
        ops.check_errors()
        ran = S
        break
    assert ran is not None, "the persistent kernel takes no frame between 512^2 and 256^2"
    with torch.no_grad():
        ref = O.dynca_nsteps(x0.double(), cond.double(), list(us), _f64(prm), pad, rate, scales=(0, 1) if two else (0,))
    e = _rel(out, ref)
    _say(f"persistent C={C} fc={fc} {'two' if two else 'one'}-scale {pad} {ran}^2 T={Tn}", err=e, bound=REL_TOL)
    assert e < REL_TOL, e


# ================================================================================================ mask plumbing at scale
def test_philox_uniform_bit_exact_at_full_size(ops):
    for (B, H, W, seed, step) in ((1, 2048, 2048, 7, 1), (8, 256, 256, 2 ** 40 + 17, 2 ** 33 + 5)):
        u = ops.philox_uniform(B, H, W, seed, step).cpu().numpy()
        assert np.array_equal(u, O.philox_uniform(seed, step, B, H, W)), (B, H, W)


def _torch_pack(mask):
    """{0,1} float [T, ...] -> int32 [T, ceil(n/32)], bit j of word i = cell 32 i + j"""
    Tn = mask.shape[0]
    m = mask.reshape(Tn, -1).to(torch.int64)
    n = m.shape[1]
    m = F.pad(m, (0, (-n) % 32))
    words = (m.view(Tn, -1, 32) << torch.arange(32, device=m.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def test_fire_mask_words_past_bit_2_24(ops):
    """pack_fire_mask / draw_fire_masks over 3 x 2560^2 = 19.7 M cells (words past bit 2^24, a partial last word avoided and
    one present) against a torch packing of the same uniforms"""
    for (Tn, B, H, W) in ((2, 3, 2560, 2560), (1, 1, 4099, 4099)):
        gen = torch.Generator().manual_seed(H)
        u = torch.rand(Tn, B, 1, H, W, generator=gen).to(DEV)
        for mode, rate in (("cond", 0.5), ("dynca", 0.3)):
            ref = (u.clamp(0, 1) < rate).float() if mode == "cond" else (u + rate).floor()
            bits = ops.pack_fire_mask(u, rate, mode)
            exp = _torch_pack(ref)
            assert torch.equal(bits, exp), (mode, Tn, B, H, W, int((bits != exp).nonzero()[0, 1]))
            del bits, exp, ref
        del u
        torch.manual_seed(1234)
        ref = torch.stack([torch.rand(B, 1, H, W, device=DEV) for _ in range(Tn)])
        torch.manual_seed(1234)
        bits = ops.draw_fire_masks(B, H, W, Tn, 0.5, "cond", torch.device(DEV))
        exp = _torch_pack((ref.clamp(0, 1) < 0.5).float())
        assert torch.equal(bits, exp), (Tn, B, H, W)
        del ref, bits, exp
