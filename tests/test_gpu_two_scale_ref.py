"""The two-scale DyNCA step (perception_scales = [0, 1]) and its backward against float64 at the smallest shape of every class.

Paths under test: ops.dynca_nsteps(..., two_scale=True, keep_history=True) and ops.dynca_nsteps_backward(..., two_scale=True) with
the persistent kernel switched off, i.e. ncahip_dynca_nsteps_fwd_ms_f32 (dynca_coarse_perceive_kernel + the MS instantiations of
dynca_step_fwd_kernel) and ncahip_dynca_nsteps_bwd_ms_f32 (the same plus dynca_ms_upT_kernel and the coarse_add / dy_half branches
of the stencil adjoint); ncahip_dynca_nsteps_fwd_persist_ms_f32 directly at the smallest frame it takes.  The reference is
oracle/nca_oracle.py in float64 on the device with scales=(0, 1) and the same uniforms.

Bounds: util.REPLAY_TOL (1e-5) for one step from the same input, util.REL_TOL (1e-4, the project's bar) for every state of the
free-running three steps, GTOL (2e-4 of the largest reference entry, as in test_gpu_fullsize_ref.py) for dL/dx0 and the four weight
gradients.  The plain fp32 CPU oracle differs from float64 by 3.0e-7 / 3.4e-7 / 6.1e-7 (forward / dL/dx0 / weights) at these
shapes, so a correct fp32 kernel has two orders of margin and a wrong tap weight or border index (1e-2) has none.

NOTHING is excluded.  A two-scale gate reaches 4 (t + 1) cells, which would blank these images, so the inputs are chosen instead:
every seed below was searched on the CPU so that the float64 trajectory has NO hidden pre-activation of an updated cell within
DYNCA_GATE_K of zero (nca_oracle.dynca_gate_influence counts them), and every float64 comparison asserts that count to be zero.

Every test prints its measured errors next to the bounds (-s)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_gpu_configs import rand_dynca_prm
from test_gpu_fullsize_ref import (DEV, DYNCA_GATE_K, DYNCA_NAMES, GTOL, _dyn_w, _dynca_case, _f64, _lever_entry,
                                   _perturbed, _rel, _rmax, _say)
from util import REL_TOL, REPLAY_TOL

pytestmark = pytest.mark.gpu
SCALES = (0, 1)
TN = 3
MAX_CCOND = 4       # the largest c_cond check_dynca accepts (kMaxCond, csrc/nca_capi.hip)

# The two-scale variants (DyncaFwdMs / DyncaFwdMsBf / DyncaBwdW2Ms through launch_dynca, csrc/nca_dynca_step.h) use TH x TW = 8 x 32 cell
# tiles, forward and backward, so H = 8 k + 2 / W = 32 k + 2 leave a remainder tile two cells tall / wide.
#        id            C   fc  c_cond      B  H   W
CASES = {"c1x1":      (12, 96, 2,          2, 2, 2),     # coarse grid 1 x 1: every up-sampling and coarse stencil tap lands on one cell
         "c2x2":      (12, 96, 0,          1, 4, 4),     # smallest shape reflect admits; no conditioning on the backward
         "c5":        (5, 24, 0,           3, 2, 6),     # C % 4 != 0, padded hidden units, B = 3, coarse 1 x 3
         "odd3x5":    (8, 40, 1,           1, 6, 10),    # odd coarse sizes, image smaller than one tile
         "rem12":     (12, 96, 3,          2, 10, 34),   # full tile + a 2-row and a 2-column remainder tile
         "rem16":     (16, 128, 3,         1, 18, 66),   # the same in the 16/128 instantiation, three tile rows
         "c13":       (13, 104, 0,         2, 8, 32),    # exactly one tile; 16/128 kernel with three padded channels
         "fc128":     (12, 128, 2,         1, 14, 30),   # C <= 12 but fc > 96: 16/128 kernel with four padded channels
         "cond4":     (16, 128, MAX_CCOND, 1, 24, 40),   # all conditioning lanes in use
         "persist":   (12, 96, 2,          1, 16, 64)}   # smallest class the persistent two-scale kernel takes (H, W % 16 == 0)
PRM_SEED = {k: 500 + i for i, k in enumerate(CASES)}

# input seeds (x0, cond, uniforms, cotangent: _dynca_inputs) with zero gates within DYNCA_GATE_K, found on the CPU in float64
SEEDS = {
    ("c1x1", "constant"): 1000,
    ("c1x1", "replicate"): 1400,
    ("c1x1", "circular"): 1800,
    ("c2x2", "constant"): 2200,
    ("c2x2", "replicate"): 2600,
    ("c2x2", "circular"): 3000,
    ("c2x2", "reflect"): 3400,
    ("c5", "constant"): 3800,
    ("c5", "replicate"): 4200,
    ("c5", "circular"): 4600,
    ("odd3x5", "constant"): 5000,
    ("odd3x5", "replicate"): 5400,
    ("odd3x5", "circular"): 5800,
    ("odd3x5", "reflect"): 6200,
    ("rem12", "constant"): 6603,
    ("rem12", "replicate"): 7000,
    ("rem12", "circular"): 7401,
    ("rem12", "reflect"): 7800,
    ("rem16", "constant"): 8201,
    ("rem16", "replicate"): 8622,
    ("rem16", "circular"): 9006,
    ("rem16", "reflect"): 9452,
    ("c13", "constant"): 9803,
    ("c13", "replicate"): 10200,
    ("c13", "circular"): 10600,
    ("c13", "reflect"): 11000,
    ("fc128", "constant"): 11400,
    ("fc128", "replicate"): 11800,
    ("fc128", "circular"): 12202,
    ("fc128", "reflect"): 12601,
    ("cond4", "constant"): 13002,
    ("cond4", "replicate"): 13417,
    ("cond4", "circular"): 13809,
    ("cond4", "reflect"): 14211,
    ("persist", "constant"): 14603,
    ("persist", "replicate"): 15004,
    ("persist", "circular"): 15403,
    ("persist", "reflect"): 15802,
}
# (case, pad, update_rate) -> seed for the runs whose fire masks differ from the table above
RATE_SEEDS = {
    ("odd3x5", "circular", 1.0): 30000,
    ("odd3x5", "circular", 0.25): 30400,
}
# (case, pad) -> seed of x0 / cond / cotangent for the in-kernel Philox masks (PHILOX_SEED, step0 = PHILOX_STEP0)
PHILOX_SEEDS = {
    ("rem12", "replicate"): 40002,
    ("odd3x5", "reflect"): 40400,
}
PHILOX_SEED, PHILOX_STEP0 = 0x5EED0001, 5


def admits(case, pad):
    _, _, _, _, H, W = CASES[case]
    return pad != "reflect" or (H >= 4 and W >= 4)


CASE_PADS = [(c, p) for c in CASES for p in O.PAD_MODES if admits(c, p)]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=False) as o:
        yield o


def make_inputs(case, seed, device=DEV):
    """(prm, x0, cond or None, us [T,B,1,H,W], cot) of a case, all from literal seeds"""
    C, fc, cc, B, H, W = CASES[case]
    prm = rand_dynca_prm(C, fc, cc, seed=PRM_SEED[case], scale=3.0)
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen) * 2 - 1
    us = torch.rand(TN, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    return prm, x0.to(device), (cond.to(device) if cc else None), us.to(device), cot.to(device)


def gate_count(prm64, x0, cond, us, pad, rate):
    c64 = None if cond is None else cond.double()
    return int(O.dynca_gate_influence(x0.double(), c64, list(us), prm64, pad, DYNCA_GATE_K, rate, scales=SCALES)[1].sum())


# ---- a local float64 copy of the two-scale step whose coarse pad mode and blend can be changed (negative controls) ------------
def _up2(y, swap=False):
    """bilinear x2 up-sampling, align_corners = False, even sizes: fine 2k <- 0.25 y[k-1] + 0.75 y[k], 2k+1 <- 0.75 y[k] + 0.25 y[k+1],
    indices clamped; swap exchanges the two lambdas"""
    near, far = (0.25, 0.75) if swap else (0.75, 0.25)
    for dim in (2, 3):
        n = y.shape[dim]
        k = torch.arange(n, device=y.device)
        prev, nxt = y.index_select(dim, (k - 1).clamp_min(0)), y.index_select(dim, (k + 1).clamp_max(n - 1))
        y = torch.stack([far * prev + near * y, near * y + far * nxt], dim=dim + 1).flatten(dim, dim + 1)
    return y


def local_step(x, cond, u, p, pad, rate, coarse_pad=None, swap=False):
    h, w = x.shape[2:]
    xc = F.interpolate(x, size=(h // 2, w // 2), mode="bilinear", align_corners=False)
    y = (O.dynca_perceive(x, pad) + _up2(O.dynca_perceive(xc, coarse_pad or pad), swap)) / 2
    if cond is not None:
        y = torch.cat([y, cond], dim=1)
    hid = F.relu(O._conv1x1(y, p["w1.weight"], p["w1.bias"]))
    return x + O._conv1x1(hid, p["w2.weight"], p["w2.bias"]) * (u + rate).floor()


def reference(prm64, x0, cond, us, pad, rate, cots, step=None):
    """float64 states x_1 .. x_T and the gradients of sum_t <x_t, cots[t]> (cots[t] None = no cotangent on x_t; t = 1 .. T) with
    respect to x0 and the four weight tensors; step=None runs the oracle's own loop"""
    x = x0.double().clone().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in prm64.items()}
    c64 = None if cond is None else cond.double()
    if step is None:
        states = O.dynca_nsteps(x, c64, list(us), p, pad, rate, scales=SCALES, collect=True)[1]
    else:
        states, xi = [], x
        for u in us:
            xi = step(xi, c64, u, p, pad, rate)
            states.append(xi)
    sum((s * g.double()).sum() for s, g in zip(states, cots) if g is not None).backward()
    grads = {"x0": x.grad}
    grads.update({k: p[n].grad.reshape(p[n].shape[0], -1) if p[n].dim() > 1 else p[n].grad for k, n in DYNCA_NAMES.items()})
    return [s.detach() for s in states], grads


def kernels(ops, prm, x0, cond, us, cot, pad, rate, **kw):
    """the per-step two-scale kernels: every state of TN steps and the backward of <x_T, cot>"""
    w = _dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0, TN, cond, us, w, pad, rate, keep_history=True, two_scale=True, **kw)
    g = ops.dynca_nsteps_backward(states, cond, us, w, cot, None, TN, pad, rate, two_scale=True, **kw)
    ops.check_errors()
    return states, g


def errors(states, g, ref_states, ref_g):
    e = {"step1": _rel(states[1], ref_states[0]), "free": max(_rel(states[t + 1], ref_states[t]) for t in range(len(ref_states)))}
    e.update({k: _rmax(g[k], ref_g[k]) for k in ("x0", "w1", "b1", "w2", "b2")})
    return e


def check(case, e):
    _say(case, **{k: float(v) for k, v in e.items()}, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] <= REPLAY_TOL, e
    assert e["free"] < REL_TOL, e
    for k in ("x0", "w1", "b1", "w2", "b2"):
        assert e[k] < GTOL, (k, e)


_RUNS = {}


def run(ops, case, pad):
    """inputs, kernel results and float64 reference of one (case, pad) of the table: computed once, shared, left unchanged"""
    if (case, pad) not in _RUNS:
        prm, x0, cond, us, cot = make_inputs(case, SEEDS[case, pad])
        p64 = _f64(prm)
        gates = gate_count(p64, x0, cond, us, pad, 0.5)
        states, g = kernels(ops, prm, x0, cond, us, cot, pad, 0.5)
        ref_states, ref_g = reference(p64, x0, cond, us, pad, 0.5, [None] * (TN - 1) + [cot])
        _RUNS[case, pad] = dict(prm=prm, p64=p64, x0=x0, cond=cond, us=us, cot=cot, gates=gates, states=states, g=g,
                                ref_states=ref_states, ref_g=ref_g)
    return _RUNS[case, pad]


# ================================================================================================ every shape class, every pad mode
@pytest.mark.parametrize("case,pad", CASE_PADS)
def test_two_scale_vs_float64(ops, case, pad):
    """one step, three free-running steps (every stored state) and the backward of every case of the table, nothing excluded"""
    r = run(ops, case, pad)
    assert r["gates"] == 0, f"seed {SEEDS[case, pad]} puts {r['gates']} gates within {DYNCA_GATE_K} of zero: pick another"
    check(f"two-scale {case} {CASES[case]} {pad}", errors(r["states"], r["g"], r["ref_states"], r["ref_g"]))


@pytest.mark.parametrize("pad", ["replicate", "circular"])
def test_persistent_smallest_frame_vs_float64(ops, pad):
    """ncahip_dynca_nsteps_fwd_persist_ms_f32 called directly (no fall-back) at 16 x 64: float64, and the per-step kernels' bits"""
    from ncahip import _capi
    r = run(ops, "persist", pad)
    assert r["gates"] == 0
    C, fc, cc, B, H, W = CASES["persist"]
    L, w, x0, cond, us = ops.lib(), _dyn_w(ops, r["prm"], r["x0"]), r["x0"], r["cond"], r["us"]
    nbytes = L.ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, cc)
    assert nbytes > 0
    ws, epoch = ops._persist_workspace(nbytes, x0.device)
    out = torch.empty_like(x0)
    rc = L.ncahip_dynca_nsteps_fwd_persist_ms_f32(ops._p(x0), ops._p(out), TN, ops._p(cond), ops._p(us), ops._p(w.w1), ops._p(w.b1),
                                                  ops._p(w.w2), ops._p(w.b2), B, C, H, W, fc, cc, ops.PAD_MODES[pad], 0.5, 0, 0,
                                                  ops._p(ws), nbytes, epoch, ops._stream())
    _capi.check(rc, "dynca_nsteps_fwd_persist_ms")
    torch.cuda.synchronize()
    ops.check_errors()
    e = _rel(out, r["ref_states"][-1])
    _say(f"persistent two-scale 16x64 {pad}", err=e, bound=REL_TOL, equals_per_step=bool(torch.equal(out, r["states"][TN])))
    assert e < REL_TOL, e
    assert torch.equal(out, r["states"][TN])


def test_dynca_case_helper_two_scale(ops):
    """test_gpu_fullsize_ref._dynca_case with scales_two=True (tile and generic switch, gate-region bookkeeping) on the table's
    remainder-tile case: with zero gates its region is empty and its bounds hold everywhere"""
    r = run(ops, "rem12", "replicate")
    assert r["gates"] == 0
    _dynca_case(ops, "two-scale rem12 replicate via _dynca_case", r["prm"], r["x0"], r["cond"], r["us"], r["cot"], "replicate",
                scales_two=True)


# ================================================================================================ negative controls
CONTROL = "rem12"


def test_control_one_weight_entry(ops):
    """the reference with ONE entry of w2.weight scaled by 1 + 1e-3 must miss the bounds"""
    r = run(ops, CONTROL, "circular")
    assert r["gates"] == 0
    p64, x0, cond, us = r["p64"], r["x0"], r["cond"], r["us"]
    with torch.no_grad():
        y = O.dynca_step(x0.double(), None if cond is None else cond.double(), us[0], p64, "circular", 0.5, SCALES, return_all=True)["y"]
        idx = _lever_entry(p64["w2.weight"], F.relu(O._conv1x1(y, p64["w1.weight"], p64["w1.bias"])))
    bad = _f64(_perturbed(r["prm"], "w2.weight", idx))
    e = errors(r["states"], r["g"], *reference(bad, x0, cond, us, "circular", 0.5, [None] * (TN - 1) + [r["cot"]]))
    _say(f"control w2.weight[{idx}] * (1 + 1e-3)", **e, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["free"] > REL_TOL, e
    assert max(e[k] for k in ("x0", "w1", "b1", "w2", "b2")) > GTOL, e


def _local_matches_oracle(r, pad):
    """the local float64 step IS the oracle's when nothing is changed (else the two controls below would prove nothing)"""
    ref_states, ref_g = reference(r["p64"], r["x0"], r["cond"], r["us"], pad, 0.5, [None] * (TN - 1) + [r["cot"]], step=local_step)
    assert _rel(ref_states[-1], r["ref_states"][-1]) < 1e-12
    assert max(_rmax(ref_g[k], r["ref_g"][k]) for k in ref_g) < 1e-10


@pytest.mark.parametrize("pad", ["circular", "constant", "reflect"])
def test_control_coarse_border(ops, pad):
    """the reference with `replicate` on the COARSE level only must miss the bounds: the test sees the coarse border"""
    r = run(ops, CONTROL, pad)
    assert r["gates"] == 0
    _local_matches_oracle(r, pad)
    step = lambda x, c, u, p, pd, rate: local_step(x, c, u, p, pd, rate, coarse_pad="replicate")
    e = errors(r["states"], r["g"], *reference(r["p64"], r["x0"], r["cond"], r["us"], pad, 0.5, [None] * (TN - 1) + [r["cot"]], step=step))
    _say(f"control coarse level replicate, kernel {pad}", **e, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] > REPLAY_TOL and e["free"] > REL_TOL, e
    assert e["x0"] > GTOL and e["w1"] > GTOL, e


def test_control_swapped_lambdas(ops):
    """the reference with the bilinear lambdas 0.25 and 0.75 exchanged must miss the bounds: the test sees the blend"""
    r = run(ops, CONTROL, "replicate")
    assert r["gates"] == 0
    _local_matches_oracle(r, "replicate")
    step = lambda x, c, u, p, pd, rate: local_step(x, c, u, p, pd, rate, swap=True)
    e = errors(r["states"], r["g"], *reference(r["p64"], r["x0"], r["cond"], r["us"], "replicate", 0.5, [None] * (TN - 1) + [r["cot"]],
                                               step=step))
    _say("control lambdas swapped", **e, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] > REPLAY_TOL and e["free"] > REL_TOL, e
    assert e["x0"] > GTOL and e["w1"] > GTOL, e


# ================================================================================================ masks, rates, cotangents
@pytest.mark.parametrize("case,pad", list(PHILOX_SEEDS))
def test_in_kernel_philox_mask(ops, case, pad):
    """us=None: forward and backward draw the masks in the kernel (seed, step0 + t); the reference is fed ops.philox_uniform"""
    C, fc, cc, B, H, W = CASES[case]
    prm, x0, cond, _, cot = make_inputs(case, PHILOX_SEEDS[case, pad])
    us = torch.stack([ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0 + t) for t in range(TN)])
    p64 = _f64(prm)
    assert gate_count(p64, x0, cond, us, pad, 0.5) == 0
    assert 0.2 < float((us + 0.5).floor().mean()) < 0.8
    states, g = kernels(ops, prm, x0, cond, None, cot, pad, 0.5, seed=PHILOX_SEED, step0=PHILOX_STEP0)
    check(f"two-scale philox {case} {pad}", errors(states, g, *reference(p64, x0, cond, us, pad, 0.5, [None] * (TN - 1) + [cot])))
    fed, gf = kernels(ops, prm, x0, cond, us, cot, pad, 0.5)                 # the same masks as explicit uniforms: the same bits
    assert torch.equal(states, fed) and all(torch.equal(g[k], gf[k]) for k in g)


@pytest.mark.parametrize("rate", [1.0, 0.25])
def test_update_rates(ops, rate):
    case, pad = "odd3x5", "circular"
    prm, x0, cond, us, cot = make_inputs(case, RATE_SEEDS[case, pad, rate])
    p64 = _f64(prm)
    assert gate_count(p64, x0, cond, us, pad, rate) == 0
    fired = float((us + rate).floor().mean())
    assert fired == 1.0 if rate == 1.0 else 0.1 < fired < 0.4
    states, g = kernels(ops, prm, x0, cond, us, cot, pad, rate)
    check(f"two-scale rate {rate} {case} {pad}", errors(states, g, *reference(p64, x0, cond, us, pad, rate, [None] * (TN - 1) + [cot])))


def test_update_rate_zero(ops):
    """no cell fires: the state comes back bit-identical, dL/dx0 is the cotangent and every weight gradient is exactly zero"""
    case, pad = "odd3x5", "circular"
    prm, x0, cond, us, cot = make_inputs(case, 1)
    states, g = kernels(ops, prm, x0, cond, us, cot, pad, 0.0)
    for t in range(1, TN + 1):
        assert torch.equal(states[t], x0), t
    assert torch.equal(g["x0"], cot)
    for k in ("w1", "b1", "w2", "b2"):
        assert int(torch.count_nonzero(g[k])) == 0, k


def test_packed_bit_masks(ops):
    """ops.pack_fire_mask words instead of float uniforms: the same bits, forward and backward"""
    r = run(ops, "rem12", "reflect")
    bits = ops.pack_fire_mask(r["us"], 0.5, "dynca")
    states, g = kernels(ops, r["prm"], r["x0"], r["cond"], bits, r["cot"], "reflect", 0.5)
    assert torch.equal(states, r["states"])
    for k in g:
        assert torch.equal(g[k], r["g"][k]), k


@pytest.mark.parametrize("case,pad", [("rem12", "constant"), ("c13", "reflect")])
def test_intermediate_cotangents(ops, case, pad):
    """g_states: random cotangents on every intermediate state (g_final carries the last) against float64 autograd of
    sum_t <x_t, g_t>"""
    r = run(ops, case, pad)
    assert r["gates"] == 0
    gen = torch.Generator().manual_seed(77)
    gs = torch.randn(TN + 1, *r["x0"].shape, generator=gen).to(DEV)
    w = _dyn_w(ops, r["prm"], r["x0"])
    g = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], w, gs[TN], gs, TN, pad, 0.5, two_scale=True)
    ops.check_errors()
    # x_0 is the input itself: its cotangent g_0 adds to dL/dx0 directly
    _, ref_g = reference(r["p64"], r["x0"], r["cond"], r["us"], pad, 0.5, [gs[t] for t in range(1, TN + 1)])
    ref_g["x0"] = ref_g["x0"] + gs[0].double()
    e = {k: _rmax(g[k], ref_g[k]) for k in g}
    _say(f"two-scale g_states {case} {pad}", **e, bound=GTOL)
    for k, v in e.items():
        assert v < GTOL, (k, e)


# ================================================================================================ bit-for-bit properties
def test_ring_of_two(ops):
    """keep_history=False (ring of 2, persistent kernel off): the final state of the stored history, bit for bit"""
    for case, pad in (("rem12", "circular"), ("c5", "replicate")):
        r = run(ops, case, pad)
        out, states = ops.dynca_nsteps(r["x0"], TN, r["cond"], r["us"], _dyn_w(ops, r["prm"], r["x0"]), pad, 0.5, two_scale=True)
        ops.check_errors()
        assert states is not None and states.shape[0] == 2
        assert torch.equal(out, r["states"][TN]), (case, pad)


def test_batch_independence(ops):
    """item b of a B = 3 run equals the B = 1 run of that item, bit for bit: forward and dL/dx0"""
    r = run(ops, "c5", "circular")
    assert r["x0"].shape[0] == 3
    for b in range(3):
        cond = None if r["cond"] is None else r["cond"][b:b + 1].contiguous()
        states, g = kernels(ops, r["prm"], r["x0"][b:b + 1].contiguous(), cond, r["us"][:, b:b + 1].contiguous(),
                            r["cot"][b:b + 1].contiguous(), "circular", 0.5)
        assert torch.equal(states[:, 0], r["states"][:, b]), b
        assert torch.equal(g["x0"][0], r["g"]["x0"][b]), b


def test_backward_is_deterministic(ops):
    for case, pad in (("rem16", "replicate"), ("cond4", "circular")):
        r = run(ops, case, pad)
        w = _dyn_w(ops, r["prm"], r["x0"])
        a = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], w, r["cot"], None, TN, pad, 0.5, two_scale=True)
        a = {k: v.clone() for k, v in a.items()}
        b = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], w, r["cot"], None, TN, pad, 0.5, two_scale=True)
        ops.check_errors()
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], r["g"][k]), (case, pad, k)


# ================================================================================================ reflect on a 1-wide coarse grid
@pytest.mark.parametrize("H,W", [(2, 8), (8, 2)])
def test_reflect_needs_a_2x2_coarse_grid(ops, H, W):
    """F.pad(mode='reflect') raises on a 1-wide axis, so the reference rejects reflect with a 2-cell side; the two-scale entry points
    return EINVAL (argument check, nothing is launched) and the module raises"""
    from ncahip import _capi
    from ncahip.models.dynca import DyNCA
    prm = rand_dynca_prm(12, 96, 0, seed=1)
    x0 = torch.zeros(1, 12, H, W, device=DEV)
    w = _dyn_w(ops, prm, x0)
    assert not ops.two_scale_fused_ok(12, H, W, 96, "reflect") and ops.two_scale_fused_ok(12, H, W, 96, "replicate")
    with pytest.raises(_capi.NcaHipError, match="coarse grid"):
        ops.dynca_nsteps(x0, 1, None, torch.zeros(1, 1, 1, H, W, device=DEV), w, "reflect", 0.5, keep_history=True, two_scale=True)
    with pytest.raises(_capi.NcaHipError, match="coarse grid"):
        ops.dynca_nsteps_backward(torch.zeros(2, 1, 12, H, W, device=DEV), None, torch.zeros(1, 1, 1, H, W, device=DEV), w,
                                  torch.zeros_like(x0), None, 1, "reflect", 0.5, two_scale=True)
    with pytest.raises(RuntimeError):       # F.pad's own error class in the reference
        O.dynca_step(x0.double(), None, torch.zeros(1, 1, H, W, device=DEV), _f64(prm), "reflect", 0.5, SCALES)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="reflect", conditioning=None, perception_scales=[0, 1], device=torch.device(DEV))
    assert not m._two_scale_fused(x0) and m._composed(x0)
    with pytest.raises((RuntimeError, _capi.NcaHipError)):
        m.forward_nsteps(x0, 1)


# ================================================================================================ refused calls enqueue nothing
def test_refused_single_step_enqueues_nothing(ops):
    """ncahip_dynca_step_fwd_ms_f32 with bit-packed masks and update_rate = 1.0 is refused by the bit-mask check (NCAHIP_ERANGE:
    floor(u + rate) must be 0 or 1).  Every host check runs before the first launch, so neither the coarse-perception scratch nor
    x_out is touched: both still hold their canary after a synchronise."""
    from ncahip import _capi
    B, C, H, W, fc = 1, 4, 4, 4, 16
    prm = rand_dynca_prm(C, fc, 0, seed=3)
    x = torch.rand(B, C, H, W, device=DEV) - 0.5
    w = _dyn_w(ops, prm, x)
    bits = torch.full(((B * H * W + 31) // 32,), 0x5A5A, dtype=torch.int32, device=DEV)
    canary = -1234.5
    out = torch.full_like(x, canary)
    pc = torch.full((B, 4 * C, H // 2, W // 2), canary, device=DEV)
    rc = ops.lib().ncahip_dynca_step_fwd_ms_f32(ops._p(x), ops._p(out), None, ops._p(bits), ops._p(w.w1), ops._p(w.b1), ops._p(w.w2),
                                                ops._p(w.b2), B, C, H, W, fc, 0, ops.PAD_MODES["replicate"], 1.0, _capi.SEED_U_IS_BITS, 0,
                                                ops._p(pc), ops._stream())
    torch.cuda.synchronize()
    assert rc == _capi.ERANGE, (rc, _capi.lib().ncahip_last_error())
    assert bool((pc == canary).all()), "the coarse pass ran before the call was refused"
    assert bool((out == canary).all())
