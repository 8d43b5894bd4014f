"""The single-scale DyNCA step and its backward against float64 at the smallest shape of every class: the sibling of
test_gpu_two_scale_ref.py for the path every training run and every benchmark row goes through.

Paths under test (persistent kernel off): ops.dynca_nsteps(..., keep_history=True) = ncahip_dynca_nsteps_fwd_f32 and
ops.dynca_nsteps_backward = ncahip_dynca_nsteps_bwd_f32 / _bf16 (nca_launch_dynca_step_fwd, nca_launch_dynca_step_bwd_mlp,
nca_launch_gram_rows, nca_launch_dynca_step_bwd_stencil); ncahip_dynca_step_bwd_f32 and ncahip_dynca_step_bwd_w2_f32 through ctypes.
The reference is oracle/nca_oracle.py in float64 on the device with the default scales=(0,) and the same explicit uniforms.

Bounds, the project's own for exactly this comparison: util.REPLAY_TOL (1e-5) for one step from the same input, util.REL_TOL (1e-4)
for every stored state of the free-running three steps, GTOL (2e-4 of the largest reference entry) for dL/dx0 and the four weight
gradients.  NOTHING is excluded: every input seed below was searched on the CPU so that the float64 trajectory has NO hidden
pre-activation of an updated cell within DYNCA_GATE_K of zero (nca_oracle.dynca_gate_influence counts them), and every float64
comparison asserts that count to be zero.

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
TN = 3
MAX_CCOND = 4       # the largest c_cond check_dynca accepts (kMaxCond, csrc/nca_capi.hip)
GRAD_KEYS = ("x0", "w1", "b1", "w2", "b2")

# Tiles are TH x TW = 8 x 32 cells forward and backward (launch_dynca, csrc/nca_dynca_step.h), so H = 8 k + 2 and
# W = 32 k + 2 (+ 4) leave remainder tiles.  What each row reaches, read off the four launchers; the class <CP, FC> is the smallest of
# <12,96>, <16,128>, <32,128> that covers (C, fc) (dispatch_dynca, csrc/nca_dynca_step.h), the rows write <CP, FC, HAS_COND[, ACC]>:
#   fwd   nca_launch_dynca_step_fwd (csrc/nca_dynca_fwd.hip): variant DyncaFwd, ACC = DyncaFwdAcc (later slices, classes <16,128> and
#         <32,128> only); VEC (16-byte loads) iff W % 4 == 0 and H W % 4 == 0
#   mlp   nca_launch_dynca_step_bwd_mlp (csrc/nca_dynca_bwd.hip): variant DyncaBwdW2 (fused dW2), ACC = DyncaBwdW2Acc; VEC iff W % 4 == 0
#   gram  nca_launch_gram_rows(ma = slice width, nb = 4 C + c_cond): launch_gram<RT, CT, ROWSPLIT>; ones column only at CT = 9
#   adj   nca_launch_dynca_step_bwd_stencil: dynca_step_bwd_stencil_vec_kernel iff W % 4 == 0, W >= 12, H >= 5, else the generic kernel
#        id              C   fc  c_cond      B  H   W
CASES = {"one":         (12, 96, 2,          2, 1, 1),     # single cell, every tap of every pad mode lands on it.  fwd <12,96,true> scalar; mlp <12,96,true,false> scalar; gram 96 x 50 <2,5,true>; adj generic
         "row":         (8, 32, 1,           1, 1, 5),     # H = 1.  fwd / mlp <12,96,true> scalar; gram 32 x 33 <2,2,false> (column split); adj generic
         "c5":          (5, 24, 0,           3, 2, 6),     # C % 4 != 0, padded hidden units, B = 3.  fwd <12,96,false> scalar; mlp <12,96,false,false> scalar; gram 24 x 20 <2,2,false>; adj generic
         "h4":          (12, 96, 0,          1, 4, 12),    # fwd <12,96,false> VEC, mlp <12,96,false,false> VEC; gram 96 x 48 <2,5,true>; adj still generic (H < 5)
         "w8":          (16, 128, 2,         1, 6, 8),     # fwd / mlp <16,128,true> VEC; gram 128 x 66 <2,5,true>; adj generic (W % 4 == 0 but W < 12)
         "band":        (12, 96, 3,          2, 5, 12),    # fwd / mlp <12,96,true> VEC; gram 96 x 51 <2,5,true>; adj dynca_step_bwd_stencil_vec_kernel at its smallest shape: band = 56 of 60 cells
         "rem12":       (12, 96, 3,          2, 10, 34),   # fwd / mlp <12,96,true> scalar (W % 4 != 0), 2-row and 2-column remainder tiles; gram 96 x 51 <2,5,true>; adj generic
         "rem16v":      (16, 128, 3,         1, 18, 68),   # fwd / mlp <16,128,true> VEC, 4-column remainder, three tile rows; gram 128 x 67 <2,5,true>; adj vec
         "c13":         (13, 104, 0,         2, 8, 32),    # exactly one tile.  fwd <16,128,false> VEC with three padded channels; mlp <16,128,false,false> VEC; gram 104 x 52 <2,5,true>; adj vec
         "fc128":       (12, 128, 2,         1, 14, 30),   # C <= 12 but fc > 96.  fwd / mlp <16,128,true> scalar; gram 128 x 50 <2,5,true>; adj generic
         "cond4":       (16, 128, MAX_CCOND, 1, 24, 40),   # all conditioning lanes.  fwd / mlp <16,128,true> VEC; gram 128 x 68 <2,5,true>; adj vec
         "c17":         (17, 40, 0,          1, 6, 10),    # smallest <32,128>: 15 padded channels.  fwd <32,128,false> scalar; mlp <32,128,false,false> scalar; gram 40 x 68 <1,5,true>; adj generic
         "c20":         (20, 100, 4,         1, 9, 36),    # fwd / mlp <32,128,true> VEC; gram 100 x 84 <2,9,true> with the ones column (its default); adj vec
         "c32":         (32, 128, 3,         1, 10, 34),   # full <32,128>.  fwd / mlp <32,128,true> scalar; gram 128 x 131 <2,9,true> ones column; adj generic
         "fc136":       (24, 136, 0,         1, 6, 13),    # two slices 128 + 8.  fwd <32,128,false> then <32,128,false,ACC> scalar; mlp <32,128,false,false> then <32,128,false,true>; gram 128 x 96 <2,9,true> ones column, then 8 x 96 <1,2,false>; adj generic
         "c12fc192":    (12, 192, 2,         1, 8, 32),    # C <= 12 with slices 128 + 64 (the c16 branch).  fwd <16,128,true> then <16,128,true,ACC> VEC; mlp <16,128,true,false> then <16,128,true,true> VEC; gram 128 x 50 <2,5,true>, 64 x 50 <1,5,true>; adj vec
         "fc320":       (16, 320, 2,         2, 9, 33),    # three slices 128 + 128 + 64, hipMemcpy2DAsync of w2 columns at three offsets.  fwd <16,128,true>, 2 x <16,128,true,ACC> scalar; mlp likewise; gram 2 x 128 x 66 <2,5,true>, 64 x 66 <1,5,true>; adj generic
         "c32fc256":    (32, 256, 3,         1, 10, 36),   # configs[4]'s class at its smallest.  fwd <32,128,true> then <32,128,true,ACC> VEC; mlp <32,128,true,false> then <32,128,true,true> VEC; gram 2 x 128 x 131 <2,9,true> ones column; adj vec
         # branches of the four launchers that no row above reaches, each at the smallest shape that does (reflect needs H, W >= 2)
         "c14fc132":    (14, 132, 0,         1, 3, 5),     # slices WITHOUT conditioning at C <= 16.  fwd <16,128,false> then <16,128,false,ACC> scalar; mlp <16,128,false,false> then <16,128,false,true>; gram 128 x 56 <2,5,true>, 4 x 56 <1,2,false>; adj generic
         "c20fc40":     (20, 40, 1,          1, 2, 3)}     # ma <= 64 with nb = 81 > 80.  fwd / mlp <32,128,true> scalar; gram 40 x 81 <1,9,true> ones column; adj generic
PRM_SEED = {k: 700 + i for i, k in enumerate(CASES)}

# input seeds (x0, cond, uniforms, cotangent: make_inputs) with zero gates within DYNCA_GATE_K, found on the CPU in float64
SEEDS = {
    ("one", "constant"): 1000,
    ("one", "replicate"): 1400,
    ("one", "circular"): 1800,
    ("row", "constant"): 2600,
    ("row", "replicate"): 3000,
    ("row", "circular"): 3400,
    ("c5", "constant"): 4200,
    ("c5", "replicate"): 4600,
    ("c5", "circular"): 5000,
    ("c5", "reflect"): 5400,
    ("h4", "constant"): 5800,
    ("h4", "replicate"): 6200,
    ("h4", "circular"): 6600,
    ("h4", "reflect"): 7000,
    ("w8", "constant"): 7400,
    ("w8", "replicate"): 7800,
    ("w8", "circular"): 8200,
    ("w8", "reflect"): 8600,
    ("band", "constant"): 9001,
    ("band", "replicate"): 9400,
    ("band", "circular"): 9800,
    ("band", "reflect"): 10200,
    ("rem12", "constant"): 10604,
    ("rem12", "replicate"): 11004,
    ("rem12", "circular"): 11401,
    ("rem12", "reflect"): 11801,
    ("rem16v", "constant"): 12244,
    ("rem16v", "replicate"): 12611,
    ("rem16v", "circular"): 13007,
    ("rem16v", "reflect"): 13409,
    ("c13", "constant"): 13801,
    ("c13", "replicate"): 14202,
    ("c13", "circular"): 14601,
    ("c13", "reflect"): 15001,
    ("fc128", "constant"): 15403,
    ("fc128", "replicate"): 15806,
    ("fc128", "circular"): 16204,
    ("fc128", "reflect"): 16601,
    ("cond4", "constant"): 17004,
    ("cond4", "replicate"): 17411,
    ("cond4", "circular"): 17803,
    ("cond4", "reflect"): 18202,
    ("c17", "constant"): 18600,
    ("c17", "replicate"): 19000,
    ("c17", "circular"): 19400,
    ("c17", "reflect"): 19800,
    ("c20", "constant"): 20200,
    ("c20", "replicate"): 20602,
    ("c20", "circular"): 21001,
    ("c20", "reflect"): 21404,
    ("c32", "constant"): 21800,
    ("c32", "replicate"): 22201,
    ("c32", "circular"): 22600,
    ("c32", "reflect"): 23000,
    ("fc136", "constant"): 23400,
    ("fc136", "replicate"): 23800,
    ("fc136", "circular"): 24200,
    ("fc136", "reflect"): 24600,
    ("c12fc192", "constant"): 25000,
    ("c12fc192", "replicate"): 25400,
    ("c12fc192", "circular"): 25801,
    ("c12fc192", "reflect"): 26201,
    ("fc320", "constant"): 26627,
    ("fc320", "replicate"): 27017,
    ("fc320", "circular"): 27406,
    ("fc320", "reflect"): 27820,
    ("c32fc256", "constant"): 28200,
    ("c32fc256", "replicate"): 28617,
    ("c32fc256", "circular"): 29000,
    ("c32fc256", "reflect"): 29410,
    ("c14fc132", "constant"): 29800,
    ("c14fc132", "replicate"): 30200,
    ("c14fc132", "circular"): 30600,
    ("c14fc132", "reflect"): 31001,
    ("c20fc40", "constant"): 31400,
    ("c20fc40", "replicate"): 31800,
    ("c20fc40", "circular"): 32200,
    ("c20fc40", "reflect"): 32600,
}
# (case, pad, update_rate) -> seed for the runs whose fire masks differ from the table above
RATE_SEEDS = {
    ("rem12", "reflect", 1.0): 33002,
    ("rem12", "reflect", 0.25): 33400,
}
# (case, pad) -> seed of x0 / cond / cotangent for the in-kernel Philox masks (PHILOX_SEED, step0 = PHILOX_STEP0)
PHILOX_SEEDS = {
    ("rem12", "constant"): 33802,
    ("fc320", "circular"): 34229,
}
PHILOX_SEED, PHILOX_STEP0 = 0x5EED0002, 5
# (case, pad) -> seed for the bf16 history: zero gates on the STORED (rounded) states
BF16_SEEDS = {
    ("band", "reflect"): 34601,
    ("c20", "circular"): 35005,
}


def admits(case, pad):
    _, _, _, _, H, W = CASES[case]
    return pad != "reflect" or (H >= 2 and W >= 2)      # below that the entry points refuse reflect (tests/test_capi_exports.py)


CASE_PADS = [(c, p) for c in CASES for p in O.PAD_MODES if admits(c, p)]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=False) as o:
        yield o


def make_inputs(case, seed, device=DEV, B=None):
    """(prm, x0, cond or None, us [T,B,1,H,W], cot) of a case, all from literal seeds, drawn as in test_gpu_two_scale_ref.py"""
    C, fc, cc, B0, H, W = CASES[case]
    B = B0 if B is None else B
    prm = rand_dynca_prm(C, fc, cc, seed=PRM_SEED[case], scale=3.0)
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen) * 2 - 1
    us = torch.rand(TN, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    return prm, x0.to(device), (cond.to(device) if cc else None), us.to(device), cot.to(device)


def _c64(cond):
    return None if cond is None else cond.double()


def gate_count(prm64, x0, cond, us, pad, rate):
    return int(O.dynca_gate_influence(x0.double(), _c64(cond), list(us), prm64, pad, DYNCA_GATE_K, rate)[1].sum())


def gate_count_at(prm64, states, cond, us, pad, rate):
    """gates of one step from each GIVEN state (states[t] -> step t): the bf16 history, where every step starts from a stored state"""
    return sum(gate_count(prm64, states[t], cond, us[t:t + 1], pad, rate) for t in range(us.shape[0]))


def bf16_history(prm64, x0, cond, us, pad, rate):
    """float64 emulation of the bf16-storage forward: every state rounded to bf16 when it is stored (the seed search runs this)"""
    states = [x0.bfloat16()]
    with torch.no_grad():
        for u in us:
            states.append(O.dynca_step(states[-1].double(), _c64(cond), u, prm64, pad, rate).float().bfloat16())
    return states


def reference(prm64, x0, cond, us, pad, rate, cots, step=None):
    """float64 states x_1 .. x_T and the gradients of sum_t <x_t, cots[t]> (cots[t] None = no cotangent on x_t; t = 1 .. T) with
    respect to x0 and the four weight tensors; step=None runs the oracle's own loop"""
    x = x0.double().clone().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in prm64.items()}
    c64 = _c64(cond)
    if step is None:
        states = O.dynca_nsteps(x, c64, list(us), p, pad, rate, collect=True)[1]
    else:
        states, xi = [], x
        for u in us:
            xi = step(xi, c64, u, p, pad, rate)
            states.append(xi)
    sum((s * g.double()).sum() for s, g in zip(states, cots) if g is not None).backward()
    return [s.detach() for s in states], _grads(x, p)


def _grads(x, p):
    g = {"x0": x.grad}
    g.update({k: p[n].grad.reshape(p[n].shape[0], -1) if p[n].dim() > 1 else p[n].grad for k, n in DYNCA_NAMES.items()})
    return g


def reference_at_states(prm64, states, cond, us, pad, rate, cot):
    """the chain of per-step float64 VJPs evaluated AT the given states (what a backward over a stored, rounded history computes):
    g_T = cot, g_t = (d step(x_t) / d x_t)^T g_{t+1}, the weight gradients summed over the steps"""
    p = {k: v.clone().requires_grad_(True) for k, v in prm64.items()}
    g = cot.double()
    for t in reversed(range(us.shape[0])):
        x = states[t].double().clone().requires_grad_(True)
        (O.dynca_step(x, _c64(cond), us[t], p, pad, rate) * g).sum().backward()      # the weights' .grad accumulates over t
        g = x.grad
    return _grads(x, p)      # x is x_0 here: its .grad is dL/dx0


def kernels(ops, prm, x0, cond, us, cot, pad, rate, g_states=None, **kw):
    """the per-step kernels: every state of TN steps and the backward of <x_T, cot> (+ sum_t <x_t, g_states[t]>)"""
    w = _dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0, TN, cond, us, w, pad, rate, keep_history=True, **kw)
    g = ops.dynca_nsteps_backward(states, cond, us, w, cot, g_states, TN, pad, rate, **kw)
    ops.check_errors()
    return states, g


def errors(states, g, ref_states, ref_g):
    e = {"step1": _rel(states[1], ref_states[0]), "free": max(_rel(states[t + 1], ref_states[t]) for t in range(len(ref_states)))}
    e.update({k: _rmax(g[k], ref_g[k]) for k in GRAD_KEYS})
    return e


def check(case, e):
    _say(case, **{k: float(v) for k, v in e.items()}, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] <= REPLAY_TOL, e
    assert e["free"] < REL_TOL, e
    for k in GRAD_KEYS:
        assert e[k] < GTOL, (k, e)


def check_grads(case, g, ref_g):
    e = {k: _rmax(g[k], ref_g[k]) for k in GRAD_KEYS}
    _say(case, **e, bound=GTOL)
    for k, v in e.items():
        assert v < GTOL, (k, e)


def last_cot(cot):
    return [None] * (TN - 1) + [cot]


_RUNS = {}


def run(ops, case, pad):
    """inputs, kernel results and float64 reference of one (case, pad) of the table: computed once, shared, left unchanged"""
    if (case, pad) not in _RUNS:
        prm, x0, cond, us, cot = make_inputs(case, SEEDS[case, pad])
        p64 = _f64(prm)
        gates = gate_count(p64, x0, cond, us, pad, 0.5)
        states, g = kernels(ops, prm, x0, cond, us, cot, pad, 0.5)
        ref_states, ref_g = reference(p64, x0, cond, us, pad, 0.5, last_cot(cot))
        _RUNS[case, pad] = dict(prm=prm, p64=p64, x0=x0, cond=cond, us=us, cot=cot, gates=gates, states=states, g=g,
                                ref_states=ref_states, ref_g=ref_g)
    return _RUNS[case, pad]


def _pick(case, pad):
    return f"seed {SEEDS[case, pad]} puts gates within {DYNCA_GATE_K} of zero: pick another"


# ================================================================================================ every shape class, every pad mode
@pytest.mark.parametrize("case,pad", CASE_PADS)
def test_dynca_vs_float64(ops, case, pad):
    """one step, three free-running steps (every stored state) and the backward of every case of the table, nothing excluded"""
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    check(f"dynca {case} {CASES[case]} {pad}", errors(r["states"], r["g"], r["ref_states"], r["ref_g"]))


@pytest.mark.parametrize("case,pad", [("rem12", "replicate"), ("cond4", "circular"), ("c32fc256", "reflect")])
def test_both_kernel_families(ops, case, pad):
    """three rows that differ in kernel family (12/96, 16/128, sliced 32/128) through test_gpu_fullsize_ref._dynca_case, which runs
    the forward under force_generic(0) and force_generic(1): with zero gates its region is empty and its bounds hold everywhere"""
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    _dynca_case(ops, f"dynca {case} {pad} via _dynca_case", r["prm"], r["x0"], r["cond"], r["us"], r["cot"], pad)


# ================================================================================================ negative controls
def test_control_one_weight_entry(ops):
    """the reference with ONE entry of w2.weight scaled by 1 + 1e-3 must miss the bounds"""
    case, pad = "rem12", "circular"
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    p64, x0, cond, us = r["p64"], r["x0"], r["cond"], r["us"]
    with torch.no_grad():
        y = O.dynca_step(x0.double(), _c64(cond), us[0], p64, pad, 0.5, return_all=True)["y"]
        idx = _lever_entry(p64["w2.weight"], F.relu(O._conv1x1(y, p64["w1.weight"], p64["w1.bias"])))
    bad = _f64(_perturbed(r["prm"], "w2.weight", idx))
    e = errors(r["states"], r["g"], *reference(bad, x0, cond, us, pad, 0.5, last_cot(r["cot"])))
    _say(f"control w2.weight[{idx}] * (1 + 1e-3)", **e, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["free"] > REL_TOL, e
    assert max(e[k] for k in GRAD_KEYS) > GTOL, e


def test_control_pad_mode(ops):
    """the reference stepped with `replicate` while the kernels run `reflect` must miss the bounds: the test sees the border"""
    case = "band"
    r = run(ops, case, "reflect")
    assert r["gates"] == 0, _pick(case, "reflect")
    e = errors(r["states"], r["g"], *reference(r["p64"], r["x0"], r["cond"], r["us"], "replicate", 0.5, last_cot(r["cot"])))
    _say("control reference replicate, kernel reflect", **e, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] > REPLAY_TOL and e["free"] > REL_TOL, e
    assert e["x0"] > GTOL and e["w1"] > GTOL, e


def local_step(x, cond, u, p, pad, rate, drop=0):
    """a float64 step whose hidden layer leaves out its last `drop` units (drop = 0: the oracle's step)"""
    y = O.dynca_perceive(x, pad)
    if cond is not None:
        y = torch.cat([y, cond], dim=1)
    fc = p["w1.weight"].shape[0] - drop
    hid = F.relu(O._conv1x1(y, p["w1.weight"][:fc], p["w1.bias"][:fc]))
    return x + O._conv1x1(hid, p["w2.weight"][:, :fc], p["w2.bias"]) * (u + rate).floor()


def test_control_lost_last_slice(ops):
    """the reference without the last 8 hidden units of fc = 136 (what a lost final slice would compute) must miss the bounds, in
    the states and in w1, b1 and w2"""
    case, pad = "fc136", "replicate"
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    args = (r["p64"], r["x0"], r["cond"], r["us"], pad, 0.5, last_cot(r["cot"]))
    same_states, same_g = reference(*args, step=local_step)       # the local step IS the oracle's when nothing is dropped
    assert _rel(same_states[-1], r["ref_states"][-1]) < 1e-12
    assert max(_rmax(same_g[k], r["ref_g"][k]) for k in same_g) < 1e-10
    e = errors(r["states"], r["g"], *reference(*args, step=lambda x, c, u, p, pd, rate: local_step(x, c, u, p, pd, rate, drop=8)))
    _say("control hidden units 128..135 dropped", **e, step_bound=REPLAY_TOL, fwd_bound=REL_TOL, grad_bound=GTOL)
    assert e["step1"] > REPLAY_TOL and e["free"] > REL_TOL, e
    assert e["w1"] > GTOL and e["b1"] > GTOL and e["w2"] > GTOL, e


# ================================================================================================ masks, rates, cotangents
@pytest.mark.parametrize("rate", [1.0, 0.25])
def test_update_rates(ops, rate):
    case, pad = "rem12", "reflect"
    prm, x0, cond, us, cot = make_inputs(case, RATE_SEEDS[case, pad, rate])
    p64 = _f64(prm)
    assert gate_count(p64, x0, cond, us, pad, rate) == 0, "pick another seed"
    fired = float((us + rate).floor().mean())
    assert fired == 1.0 if rate == 1.0 else 0.1 < fired < 0.4
    states, g = kernels(ops, prm, x0, cond, us, cot, pad, rate)
    check(f"dynca rate {rate} {case} {pad}", errors(states, g, *reference(p64, x0, cond, us, pad, rate, last_cot(cot))))


@pytest.mark.parametrize("case,pad", [("rem12", "constant"), ("fc320", "circular")])
def test_in_kernel_philox_mask(ops, case, pad):
    """us=None: forward and backward draw the masks in the kernel (seed, step0 + t), every hidden-layer slice of fc = 320 anew; the
    reference is fed ops.philox_uniform of the same key, so a slice that drew another mask misses the float64 bounds"""
    C, fc, cc, B, H, W = CASES[case]
    prm, x0, cond, _, cot = make_inputs(case, PHILOX_SEEDS[case, pad])
    us = torch.stack([ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0 + t) for t in range(TN)])
    for t in range(TN):
        assert (us[t].cpu().numpy() == O.philox_uniform(PHILOX_SEED, PHILOX_STEP0 + t, B, H, W)).all(), t
    p64 = _f64(prm)
    assert gate_count(p64, x0, cond, us, pad, 0.5) == 0, "pick another seed"
    assert 0.2 < float((us + 0.5).floor().mean()) < 0.8
    states, g = kernels(ops, prm, x0, cond, None, cot, pad, 0.5, seed=PHILOX_SEED, step0=PHILOX_STEP0)
    check(f"dynca philox {case} {pad}", errors(states, g, *reference(p64, x0, cond, us, pad, 0.5, last_cot(cot))))
    fed, gf = kernels(ops, prm, x0, cond, us, cot, pad, 0.5)                 # the same masks as explicit uniforms: the same bits
    assert torch.equal(states, fed) and all(torch.equal(g[k], gf[k]) for k in g)


@pytest.mark.parametrize("case,pad", [("band", "circular"), ("fc136", "reflect")])
def test_packed_bit_masks(ops, case, pad):
    """ops.pack_fire_mask words instead of float uniforms: the same bits, forward and backward"""
    r = run(ops, case, pad)
    bits = ops.pack_fire_mask(r["us"], 0.5, "dynca")
    states, g = kernels(ops, r["prm"], r["x0"], r["cond"], bits, r["cot"], pad, 0.5)
    assert torch.equal(states, r["states"])
    for k in g:
        assert torch.equal(g[k], r["g"][k]), k


@pytest.mark.parametrize("case,pad", [("band", "constant"), ("c20", "reflect")])
def test_intermediate_cotangents(ops, case, pad):
    """g_states: non-zero cotangents on the states t = 1, 2 (g_final carries the last) against float64 autograd of sum_t <x_t, cot_t>"""
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    gen = torch.Generator().manual_seed(78)
    gs = torch.randn(TN + 1, *r["x0"].shape, generator=gen).to(DEV)
    gs[0] = 0
    g = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], _dyn_w(ops, r["prm"], r["x0"]), gs[TN], gs, TN, pad, 0.5)
    ops.check_errors()
    _, ref_g = reference(r["p64"], r["x0"], r["cond"], r["us"], pad, 0.5, [gs[t] for t in range(1, TN + 1)])
    check_grads(f"dynca g_states {case} {pad}", g, ref_g)
    assert max(_rmax(g[k], r["ref_g"][k]) for k in GRAD_KEYS) > 10 * GTOL        # the intermediate cotangents carry weight


# ================================================================================================ the unfused entry point
@pytest.mark.parametrize("case,pad", [("c17", "reflect"), ("rem16v", "circular")])
def test_unfused_step_backward(ops, case, pad):
    """ncahip_dynca_step_bwd_f32 (h, dh, dL/dy and dL/dx in buffers) of the table's first step against the float64 VJP of
    nca_oracle.dynca_step, and bit for bit against ncahip_dynca_step_bwd_w2_f32"""
    from ncahip import _capi
    r = run(ops, case, pad)
    assert r["gates"] == 0, _pick(case, pad)
    C, fc, cc, B, H, W = CASES[case]
    x0, cond, u, gn, p64 = r["x0"], r["cond"], r["us"][0].contiguous(), r["cot"], r["p64"]
    w = _dyn_w(ops, r["prm"], x0)
    L, P, pm = ops.lib(), ops._p, ops.PAD_MODES[pad]
    hb, dh, dy, gx = (torch.empty(B, fc, H, W, device=DEV), torch.empty(B, fc, H, W, device=DEV),
                      torch.empty(B, 4 * C, H, W, device=DEV), torch.empty_like(gn))
    _capi.check(L.ncahip_dynca_step_bwd_f32(P(x0), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, pm, 0.5,
                                            0, 0, P(gn), P(gx), P(hb), P(dh), P(dy), ops._stream()), "bwd")
    dh2, dy2, gx2, out = torch.empty_like(dh), torch.empty_like(dy), torch.empty_like(gn), torch.empty(C * fc + C, device=DEV)
    nws = L.ncahip_dynca_step_bwd_w2_workspace(B, C, H, W, fc)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    _capi.check(L.ncahip_dynca_step_bwd_w2_f32(P(x0), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, pm, 0.5,
                                               0, 0, P(gn), P(gx2), P(dh2), P(dy2), P(out), 0, P(ws), nws, ops._stream()), "bwd_w2")
    ops.check_errors()
    # float64: autograd gives dL/dx and dL/dy; h and dh written out, and tied to autograd through dL/dy = w1^T dh
    x = x0.double().clone().requires_grad_(True)
    s = O.dynca_step(x, _c64(cond), u, p64, pad, 0.5, return_all=True)
    gx_ref, gy_ref = torch.autograd.grad((s["x"] * gn.double()).sum(), [x, s["y"]])
    with torch.no_grad():
        pre = O._conv1x1(s["y"], p64["w1.weight"], p64["w1.bias"])
        h_ref = F.relu(pre)
        dh_ref = torch.einsum("cf,bchw->bfhw", p64["w2.weight"][:, :, 0, 0], gn.double() * s["m"]) * (pre > 0)
        assert _rmax(torch.einsum("fk,bfhw->bkhw", p64["w1.weight"][:, :, 0, 0], dh_ref), gy_ref) < 1e-12
    e = {"g_x": _rmax(gx, gx_ref), "h": _rmax(hb, h_ref), "dh": _rmax(dh, dh_ref), "dy": _rmax(dy, gy_ref[:, :4 * C])}
    e_h = _rel(hb, h_ref)
    _say(f"unfused step backward {case} {pad}", **e, bound=GTOL, h_vs_hidden=e_h, h_bound=REPLAY_TOL)
    for k, v in e.items():
        assert v < GTOL, (k, e)
    assert e_h <= REPLAY_TOL, e_h
    assert torch.equal(gx, gx2) and torch.equal(dh, dh2)


# ================================================================================================ bf16 history
@pytest.mark.parametrize("case,pad", [("band", "reflect"), ("c20", "circular")])
def test_bf16_history_backward(ops, case, pad):
    """ncahip_dynca_nsteps_bwd_bf16 differentiates at the stored, rounded states: the reference is the chain of per-step float64 VJPs
    evaluated at the states the forward stored (downloaded and widened exactly), with zero gates counted on those same states"""
    prm, x0, cond, us, cot = make_inputs(case, BF16_SEEDS[case, pad])
    p64 = _f64(prm)
    w = _dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0.bfloat16(), TN, cond, us, w, pad, 0.5, keep_history=True)
    assert states.dtype == torch.bfloat16 and states.shape[0] == TN + 1
    g = ops.dynca_nsteps_backward(states, cond, us, w, cot, None, TN, pad, 0.5)
    ops.check_errors()
    assert gate_count_at(p64, states, cond, us, pad, 0.5) == 0, "a gate on the device's stored states: pick another seed"
    emu = bf16_history(p64, x0, cond, us, pad, 0.5)
    flips = sum(int((states[t] != emu[t]).sum()) for t in range(TN + 1))       # final-rounding flips against the float64 emulation
    check_grads(f"dynca bf16 history {case} {pad} (stored elements that differ from the emulation: {flips})", g,
                reference_at_states(p64, states, cond, us, pad, 0.5, cot))


# ================================================================================================ bit-for-bit properties
def test_batch_independence(ops):
    """item 0 of the B = 2 run equals the B = 1 run of that item, bit for bit: every state and dL/dx0"""
    r = run(ops, "rem12", "circular")
    assert r["x0"].shape[0] == 2
    states, g = kernels(ops, r["prm"], r["x0"][:1].contiguous(), r["cond"][:1].contiguous(), r["us"][:, :1].contiguous(),
                        r["cot"][:1].contiguous(), "circular", 0.5)
    assert torch.equal(states[:, 0], r["states"][:, 0])
    assert torch.equal(g["x0"][0], r["g"]["x0"][0])


def test_backward_is_deterministic(ops):
    """two identical calls give identical bits in all five gradients"""
    for case, pad in (("rem12", "replicate"), ("fc320", "constant")):
        r = run(ops, case, pad)
        w = _dyn_w(ops, r["prm"], r["x0"])
        a = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], w, r["cot"], None, TN, pad, 0.5)
        a = {k: v.clone() for k, v in a.items()}
        b = ops.dynca_nsteps_backward(r["states"], r["cond"], r["us"], w, r["cot"], None, TN, pad, 0.5)
        ops.check_errors()
        for k in GRAD_KEYS:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], r["g"][k]), (case, pad, k)
