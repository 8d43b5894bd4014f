"""ConditionedNCA grow histories replayed step by step against float64, cell by cell, nothing excluded in the forward.

Two free-running trajectories part for good at the first near-threshold cell that resolves differently, so long grows used to be
held to fraction bounds only.  The kernels record their own trajectory (keep_history=True: states slot k = the pending x'_{k-1},
pre slot k = that step's pre mask, include/ncahip.h), and nca_oracle.cond_replay_forward restarts the float64 oracle from the
GPU's own input at every step: every mask decision then compares the same fp32 numbers on both sides and is demanded exactly.
Per step k, with in_k = cond_resolve(slot k, pre slot k):

  (a) pre slot k+1 == alive(in_k) bit for bit;  (b) a cell that does not fire keeps in_k by value (firing-cell lists);
  (c) a cell that fires lies within REPLAY_TOL * max(1, max|ref|) of the float64 pending state;
  (d) x_final == cond_resolve(slot T) by value;  (e) the keep_history=False x_final (the bench's ring-2 call) equals it.

The backward is checked per step (cond_grow_backward with T = 1 on [in_k, slot k+1], g_final = the float64 replay adjoint rounded
to fp32) and chained (T steps against nca_oracle.cond_replay_vjp); the only excuse is a gradient-carrying ReLU gate within GATE_K
of zero (cond_replay_gates), which within one step sees its own cell's cotangent only.  Every case prints its worst errors and the
number of cells strictly checked whose pooled alpha lies within 1e-4 of float32(0.1) (-s)."""
import gc
import time

import pytest
import torch
import torch.nn.functional as F

import bench
from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_gpu_configs import rand_cond_prm
from test_gpu_cond_persist import _Spy
from test_gpu_fullsize_ref import COND_NAMES, GTOL, _cond_hidden2, _cond_w, _f64, _lever_entry, _perturbed, _rel2, _rmax
from util import GATE_K, REL_TOL, REPLAY_TOL, near_threshold, replay_step_check

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ULP = 2.0 ** -8
PATHS = {"default": 0, "dense": 32, "wave": 2, "generic": 1}      # ncahip_debug_force_generic bits (include/ncahip.h)


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:
        yield o


@pytest.fixture(autouse=True)
def _cost(request):
    gc.collect()
    torch.cuda.empty_cache()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[cost] {request.node.name}: {time.time() - t0:.1f} s")
    gc.collect()
    torch.cuda.empty_cache()


def _say(case, **kv):
    print(f"\n[replay] {case}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


class Draws:
    """The fire-mask source of a grow: 'uniform' (float draws), 'bits' (bit-packed masks) or 'philox' (in-kernel, keyed by seed);
    arg = what cond_grow takes, u(k) = what the replay takes for step k (1 - mask for bits), at(k) = (us, seed, step0) of step k
    alone for a T = 1 backward."""

    def __init__(self, ops, mode, B, H, W, Tn, rate, seed=42, gen_seed=0):
        self.mode, self.seed, self.ops, self.shape = mode, seed, ops, (B, H, W)
        if mode == "philox":
            self.arg = None
            return
        us = torch.rand(Tn, B, 1, H, W, generator=torch.Generator().manual_seed(gen_seed)).to(DEV)
        if mode == "uniform":
            self.arg = us
        else:
            self.arg = ops.pack_fire_mask(us, rate, "cond")
            self.mask = ops.unpack_fire_mask(self.arg, B, H, W)

    def u(self, k):
        if self.mode == "philox":
            return self.ops.philox_uniform(*self.shape, self.seed, k)
        return self.arg[k] if self.mode == "uniform" else 1.0 - self.mask[k]

    def __getitem__(self, k):
        return self.u(k)

    def at(self, k):
        if self.mode == "philox":
            return None, self.seed, k
        return self.arg[k:k + 1], self.seed, 0


def _grow(ops, path, x, Tn, goal, dr, w, alive, rate, hist):
    """cond_grow on one kernel path; 'persist' asserts that the one-launch kernel ran"""
    try:
        if path == "bf16x3":
            ops.set_cond_precision("bf16x3")
        elif path == "persist":
            ops.persistent_cond = True
        else:
            ops.force_generic(PATHS[path])
        if path == "persist":
            with _Spy(ops) as spy:
                r = ops.cond_grow(x, Tn, goal, dr.arg, w, alive, fire_rate=rate, seed=dr.seed, keep_history=hist)
            assert spy.seen and spy.seen[-1] == 0, spy.seen
        else:
            r = ops.cond_grow(x, Tn, goal, dr.arg, w, alive, fire_rate=rate, seed=dr.seed, keep_history=hist)
        torch.cuda.synchronize()
        return r
    finally:
        ops.force_generic(0)
        ops.set_cond_precision(0)
        ops.persistent_cond = False


def _replay(states, pre, out, gpad64, dr, p64, alive, rate, tol=REPLAY_TOL, flags=False):
    """(a)-(d) over the whole history; returns (worst {'pre','keep','fire','final'}, near-threshold cells, per-step bad maps)"""
    worst, near, bad = {"pre": 0, "keep": 0, "fire": 0.0, "final": 0}, 0, {}
    for rec in O.cond_replay_forward(states, pre, out, gpad64, dr, p64, alive, fire_rate=rate):
        if "x_final_got" in rec:
            worst["final"] = int((rec["x_in"] != rec["x_final_got"]).sum())
            break
        b, e = replay_step_check(rec, tol)
        worst = {"pre": worst["pre"] + e["pre"], "keep": worst["keep"] + e["keep"], "fire": max(worst["fire"], e["fire"]),
                 "final": 0}
        if alive >= 0:
            near += int(near_threshold(rec["x_in"], alive).sum()) + int((near_threshold(rec["pend_got"], alive) & rec["pre_got"]).sum())
        if flags:
            bad[rec["k"]] = b
        del rec
    return worst, near, bad


def _forward_case(ops, case, prm, x, goal, Tn, dr, paths, alive=3, rate=0.5, straddle=False):
    """every path: history + (a)-(e); a history equal to one already replayed is not replayed again (same inputs, same check)"""
    C = x.shape[1]
    w = _cond_w(ops, prm, x)
    p64 = _f64(prm)
    gpad64 = None if goal is None else O.cond_pad_goal(goal.double(), C)
    done = []
    for path in paths:
        out, states, pre = _grow(ops, path, x, Tn, goal, dr, w, alive, rate, True)
        out = out.clone()
        ring2, _, _ = _grow(ops, path, x, Tn, goal, dr, w, alive, rate, False)
        same_e = torch.equal(ring2, out)
        del ring2
        twin = next((n for n, s, p in done if torch.equal(s, states) and torch.equal(p[1:], pre[1:])), None)
        if twin is None:
            tol = REL_TOL if path == "bf16x3" else REPLAY_TOL
            worst, near, _ = _replay(states, pre, out, gpad64, dr, p64, alive, rate, tol)
            _say(f"{case} fwd [{path}]", pre_mismatch=worst["pre"], nonfiring_changed=worst["keep"], firing_worst=worst["fire"],
                 bound=tol, final_mismatch=worst["final"], ring2_equal=same_e, near_threshold_cells_checked=near)
            assert worst["pre"] == 0 and worst["keep"] == 0 and worst["final"] == 0, worst
            assert worst["fire"] <= tol, worst
            if straddle:
                assert near > 0
            done.append((path, states, pre))
        else:
            fin = O.cond_resolve(states[Tn].double(), pre[Tn], alive)
            _say(f"{case} fwd [{path}]", history_identical_to=twin, ring2_equal=same_e,
                 final_mismatch=int((fin != out.double()).sum()))
            assert torch.equal(fin, out.double())
            del states, pre
        assert same_e, f"{case} [{path}]: keep_history=False x_final differs from the recorded history's"
        del out
        ops.check_errors()
    return done


# ------------------------------------------------------------------------------------------------ forward: the bench call
def _bench_inputs(straddle):
    prm = bench.make_weights(torch.Generator().manual_seed(0))
    dgen = torch.Generator().manual_seed(1234)
    x0 = torch.rand(bench.B, bench.C, bench.H, bench.W, generator=dgen)
    goal = torch.randn(bench.B, bench.GOAL_CH, bench.H, bench.W, generator=dgen) * 0.5
    if straddle:
        x0[:, bench.ALIVE_CH] *= 0.12
    return prm, x0.to(DEV), goal.to(DEV)


@pytest.mark.parametrize("straddle", [False, True])
def test_bench_call_replayed(ops, straddle):
    """bench.py's call: 8 x 16 x 256^2, T = 64, in-kernel Philox seed 42, rate 0.5; every path that takes the shape"""
    prm, x0, goal = _bench_inputs(straddle)
    dr = Draws(ops, "philox", bench.B, bench.H, bench.W, bench.T, 0.5, seed=42)
    _forward_case(ops, f"bench 8x16x256^2 T=64{' straddling' if straddle else ''}", prm, x0, goal, bench.T, dr,
                  ["default", "dense", "wave", "generic", "bf16x3"], straddle=straddle)


# ------------------------------------------------------------------------------------------------ forward: training shape
def _train_inputs(B, C, S, seed, start):
    gen = torch.Generator().manual_seed(seed)
    if start == "seed":
        x0 = O.cond_generate_seed(B, C, 3, S)
    else:
        x0 = torch.rand(B, C, S, S, generator=gen)
        x0[:, 3] *= 0.12
    goal = torch.randn(B, C - 4, S, S, generator=gen) * 0.5
    return x0.to(DEV), goal.to(DEV)


@pytest.mark.parametrize("start", ["seed", "straddle"])
def test_training_shape_replayed(ops, start):
    """the reference's default model (C = 20, hidden 64, goal 16) at its training shape 8 x 20 x 64^2, T = 64, the persistent
    one-launch grow included"""
    prm = rand_cond_prm(20, seed=61, out_scale=1.0)
    x0, goal = _train_inputs(8, 20, 64, 610, start)
    dr = Draws(ops, "philox", 8, 64, 64, 64, 0.5, seed=7)
    _forward_case(ops, f"train 8x20x64^2 T=64 from {start}", prm, x0, goal, 64, dr,
                  ["default", "dense", "generic", "bf16x3", "persist"], straddle=start == "straddle")


def test_training_c20_256_replayed(ops):
    prm = rand_cond_prm(20, seed=62, out_scale=1.0)
    x0, goal = _train_inputs(8, 20, 256, 620, "straddle")
    dr = Draws(ops, "philox", 8, 256, 256, 32, 0.5, seed=8)
    _forward_case(ops, "8x20x256^2 T=32 straddling", prm, x0, goal, 32, dr, ["default", "dense", "generic"], straddle=True)


# ------------------------------------------------------------------------------------------------ forward: edges
EDGES = [  # (name, B, C, hidden, H, W, goal_ch, alive, rate, mask mode, T)
    ("partial super-tiles 2x16x40x72", 2, 16, 64, 40, 72, 12, 3, 0.5, "uniform", 16),
    ("C=13 hidden 48", 2, 13, 48, 32, 48, 9, 3, 0.5, "bits", 16),
    ("W=52 (4 | W, 16 does not)", 2, 16, 64, 36, 52, 12, 3, 0.5, "philox", 16),
    ("B=1", 1, 16, 64, 48, 64, 12, 3, 0.5, "bits", 16),
    ("alive_ch=-1", 2, 12, 64, 32, 32, 8, -1, 0.5, "uniform", 12),
    ("goal_ch=0", 2, 16, 64, 32, 32, 0, 3, 0.5, "philox", 16),
    ("rate 0", 2, 16, 64, 32, 32, 12, 3, 0.0, "uniform", 8),
    ("rate 0.1", 2, 16, 64, 32, 32, 12, 3, 0.1, "bits", 16),
    ("rate 1.0", 2, 16, 64, 32, 32, 12, 3, 1.0, "philox", 16),
]


@pytest.mark.parametrize("edge", EDGES, ids=[e[0] for e in EDGES])
def test_edges_replayed(ops, edge):
    name, B, C, hid, H, W, gch, alive, rate, mode, Tn = edge
    prm = rand_cond_prm(C, seed=70 + C + H, hidden=hid, out_scale=1.0)
    gen = torch.Generator().manual_seed(700 + W)
    x0 = torch.rand(B, C, H, W, generator=gen)
    if alive >= 0:
        x0[:, alive] *= 0.12
    goal = (torch.randn(B, gch, H, W, generator=gen) * 0.5).to(DEV) if gch else None
    dr = Draws(ops, mode, B, H, W, Tn, rate, seed=3, gen_seed=W)
    paths = ["default", "dense", "generic"] + (["wave"] if C <= 16 else [])
    _forward_case(ops, f"edge {name} ({mode})", prm, x0.to(DEV), goal, Tn, dr, paths, alive=alive, rate=rate,
                  straddle=alive >= 0)


# ------------------------------------------------------------------------------------------------ forward: bf16 storage
def _bf16_case(ops, case, prm, x, goal, Tn, dr):
    """each bf16 step against cond_step_bf16 from the GPU's own bf16 input: pre exact, pending within 2 ulp, < 3 % differing"""
    C = x.shape[1]
    x, goal = x.bfloat16(), goal.bfloat16()
    w = _cond_w(ops, prm, x)
    out, states, pre = ops.cond_grow(x, Tn, goal, dr.arg, w, 3, seed=dr.seed, keep_history=True)
    ring2, _, _ = ops.cond_grow(x, Tn, goal, dr.arg, w, 3, seed=dr.seed)
    ops.check_errors()
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.double(), C)
    worst, frac, near = 0.0, 0.0, 0
    for k in range(Tn):
        xin = states[0].double() if k == 0 else O.cond_resolve(states[k].double(), pre[k], 3)
        with torch.no_grad():
            _, rpre, rpend = O.cond_step_bf16(xin, gpad, dr.u(k), p64)
        assert torch.equal(rpre, pre[k + 1].bool().unsqueeze(1)), k
        got = states[k + 1].double()
        worst = max(worst, float(((got - rpend).abs() / rpend.abs().clamp_min(1.0)).max()))
        frac = max(frac, float((got != rpend).float().mean()))
        near += int(near_threshold(xin).sum())
        del xin, rpre, rpend, got
    fin = O.cond_resolve(states[Tn].double(), pre[Tn], 3)
    _say(case + " bf16 fwd", pending_worst=worst, bound=2 * ULP, differing_fraction=frac, near_threshold_cells_checked=near,
         final_equal=bool(torch.equal(fin, out.double())), ring2_equal=bool(torch.equal(ring2, out)))
    assert worst <= 2 * ULP and frac < 0.03
    assert torch.equal(fin, out.double()) and torch.equal(ring2, out)


def test_bf16_storage_replayed(ops):
    prm, x0, goal = _bench_inputs(True)
    _bf16_case(ops, "bench 8x16x256^2 T=64 straddling", prm, x0, goal, 64, Draws(ops, "philox", 8, 256, 256, 64, 0.5, seed=42))
    prm = rand_cond_prm(20, seed=63, out_scale=1.0)
    x0, goal = _train_inputs(8, 20, 64, 630, "seed")
    _bf16_case(ops, "train 8x20x64^2 T=64 from seed", prm, x0, goal, 64, Draws(ops, "philox", 8, 64, 64, 64, 0.5, seed=9))


# ------------------------------------------------------------------------------------------------ backward
def _grad_errs(g, gx, gg, gw, C, gch):
    e = {"x": _rmax(g["x0"], gx)}
    if gch:
        e["goal"] = _rmax(g["goal"], gg[:, C - gch:])
    e.update({k: _rmax(g[k], gw[n]) for k, n in COND_NAMES.items()})
    return e


def _outside(got, ref, region):
    """max |got - ref| / max |ref| over the cells outside region [B,1,H,W]"""
    d = (got.double() - ref).abs()[~region.expand_as(ref)]
    return float(d.max()) / max(float(ref.abs().max()), 1e-12) if d.numel() else 0.0


def _backward_case(ops, case, prm, x0, goal, Tn, dr, every, chain_T, forms=(24, 16, 0), control=False):
    """One float64 replay-VJP walk down the recorded history.  Every `every`-th step: the T = 1 kernel backward from the fp32-rounded
    replay adjoint, with the cotangent zeroed on cells holding an ambiguous gate (everything strict) and with the full cotangent
    (per-cell gradients strict outside those cells' 3 x 3 neighbourhood).  Then the chained kernel backward over steps
    [0, chain_T) in each form of kernel A against the replay's chain."""
    B, C, H, W = x0.shape
    gch = goal.shape[1]
    w = _cond_w(ops, prm, x0)
    out, states, pre = ops.cond_grow(x0, Tn, goal, dr.arg, w, 3, seed=dr.seed, keep_history=True)
    ops.check_errors()
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.double(), C)
    cot = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H + Tn)).to(DEV)
    acc = {"quiet": 0.0, "full": 0.0, "full_w_max": 0.0, "full_w_l2": 0.0, "gates": 0, "steps": 0}
    chain = {"g": None, "gg": None, "gw": None}
    ctl = {}

    def one_step(k, g_next):
        us, seed, step0 = dr.at(k)
        st = torch.stack([(states[0] if k == 0 else O.cond_resolve(states[k], pre[k], 3)), states[k + 1]])
        pr = torch.stack([pre[k + 1], pre[k + 1]])
        return ops.cond_grow_backward(st, pr, goal, us, w, g_next.float(), 1, 3, seed=seed, step0=step0)

    def on_step(k, x_in, g_next, r):
        gx, gg, gw = r
        if k < chain_T:
            chain["gg"] = gg if chain["gg"] is None else chain["gg"] + gg
            chain["gw"] = gw if chain["gw"] is None else {n: chain["gw"][n] + gw[n] for n in gw}
        if k == chain_T - 1:
            chain["g"] = g_next                    # dL/d in_{chain_T}: the chained check's g_final
        if k % every and k != Tn - 1:
            return
        cells, n = O.cond_replay_gates(x_in, states[k + 1], pre[k + 1], gpad, dr.u(k), p64, 3, GATE_K)
        gf = g_next.float().double()               # the kernel sees the fp32-rounded adjoint: so does its reference
        full = O.cond_replay_vjp_step(x_in, states[k + 1], pre[k + 1], gpad, dr.u(k), p64, gf, 3)
        quiet_cot = gf * ~cells
        quiet = O.cond_replay_vjp_step(x_in, states[k + 1], pre[k + 1], gpad, dr.u(k), p64, quiet_cot, 3)
        gq = one_step(k, quiet_cot)
        eq = _grad_errs(gq, *quiet, C, gch)
        g = one_step(k, gf)
        nb = F.max_pool2d(cells.float(), 3, 1, 1) > 0
        ef = max(_outside(g["x0"], full[0], nb), _outside(g["goal"], full[1][:, C - gch:], nb))
        ew = {k_: (_rmax(g[k_], full[2][n_]), _rel2(g[k_], full[2][n_])) for k_, n_ in COND_NAMES.items()}
        acc["quiet"] = max(acc["quiet"], max(eq.values()))
        acc["full"] = max(acc["full"], ef)
        acc["full_w_max"] = max(acc["full_w_max"], max(v[0] for v in ew.values()))
        acc["full_w_l2"] = max(acc["full_w_l2"], max(v[1] for v in ew.values()))
        acc["gates"] += int(n.sum())
        acc["steps"] += 1
        assert max(eq.values()) < GTOL, (k, eq)
        assert ef < GTOL, (k, ef)
        for k_, (emax, el2) in ew.items():
            if int(n.sum()) == 0:
                assert emax < GTOL, (k, k_, emax)
            else:
                assert el2 < 1e-3 and emax < 1e-2, (k, k_, emax, el2)
        if control:      # the same kernel gradients against the reference with the lever weight changed (_lever_control)
            if "bad" not in ctl:
                ctl["bad"], ctl["entry"] = _lever(prm, states, gpad)
                ctl["bwd"] = 0.0
            ref = O.cond_replay_vjp_step(x_in, states[k + 1], pre[k + 1], gpad, dr.u(k), ctl["bad"], quiet_cot, 3)
            ctl["bwd"] = max(ctl["bwd"], max(_grad_errs(gq, *ref, C, gch).values()))

    gx0, _, _ = O.cond_replay_vjp(states, pre, gpad, dr, p64, cot, 3, on_step=on_step)
    _say(case + " bwd per step", steps_checked=acc["steps"], quiet_cot_worst=acc["quiet"], full_cot_outside_gates=acc["full"],
         bound=GTOL, full_cot_weights_max=acc["full_w_max"], full_cot_weights_l2=acc["full_w_l2"], gates_excused=acc["gates"])
    # chained: the kernel backward over [0, chain_T) with g_final = the replay adjoint at chain_T
    region, cnt = O.cond_replay_gate_region(states[:chain_T + 1], pre[:chain_T + 1], gpad, dr, p64, 3, GATE_K)
    for form in forms:
        ops.force_generic(form)
        try:
            us = dr.arg if dr.arg is None else dr.arg[:chain_T]
            g = ops.cond_grow_backward(states[:chain_T + 1], pre[:chain_T + 1], goal, us, w, chain["g"].float(), chain_T, 3,
                                       seed=dr.seed)
        finally:
            ops.force_generic(0)
        ops.check_errors()
        ex, eg = _outside(g["x0"], gx0, region), _outside(g["goal"], chain["gg"][:, C - gch:], region)
        ew = {k_: (_rmax(g[k_], chain["gw"][n_]), _rel2(g[k_], chain["gw"][n_])) for k_, n_ in COND_NAMES.items()}
        _say(case + f" bwd chained T={chain_T} [force {form}]", x0_outside_region=ex, goal_outside_region=eg, bound=GTOL,
             gates=int(cnt.sum()), region_fraction=float(region.float().mean()),
             weights_max=max(v[0] for v in ew.values()), weights_l2=max(v[1] for v in ew.values()))
        assert ex < GTOL and eg < GTOL, (form, ex, eg)
        for k_, (emax, el2) in ew.items():
            if int(cnt.sum()) == 0:
                assert emax < GTOL, (form, k_, emax)
            else:
                assert el2 < 1e-3 and emax < 1e-2, (form, k_, emax, el2)
        del g
    if control:
        _lever_control(ops, case, prm, states, pre, out, gpad, dr, ctl, C, gch)


def _lever(prm, states, gpad):
    """(float64 weights with the lever entry of the output layer scaled by 1 + 1e-3, 'key[index]')"""
    p64 = _f64(prm)
    with torch.no_grad():
        x1 = states[0].double()
        p = O.cond_perceive(x1 + gpad * O._alive32(x1, 3, 0.1).double(), p64["perception_net.weight"])
        key = "update_net.out.4.weight"
        idx = _lever_entry(p64[key], _cond_hidden2(p, p64))
    return _f64(_perturbed(prm, key, idx)), f"{key}[{idx}]"


def _lever_control(ops, case, prm, states, pre, out, gpad, dr, ctl, C, gch):
    """the lever weight scaled by 1 + 1e-3 must miss the per-step forward bound and the per-step backward bound (quiet cotangent,
    worst step)"""
    worst, _, _ = _replay(states, pre, out, gpad, dr, ctl["bad"], 3, 0.5)
    _say(case + " negative control", entry=ctl["entry"], fwd_firing_worst=worst["fire"], fwd_bound=REPLAY_TOL,
         bwd_step_worst=ctl["bwd"], bwd_bound=GTOL)
    assert worst["fire"] > REPLAY_TOL and ctl["bwd"] > GTOL


def test_backward_training_shape_from_seed(ops):
    """8 x 20 x 64^2, T = 64 from cond_generate_seed: every step, and the chained T = 64 backward in the three forms of kernel A"""
    prm = rand_cond_prm(20, seed=64, out_scale=1.0)
    x0, goal = _train_inputs(8, 20, 64, 640, "seed")
    _backward_case(ops, "train 8x20x64^2 T=64 from seed", prm, x0, goal, 64, Draws(ops, "philox", 8, 64, 64, 64, 0.5, seed=11),
                   every=1, chain_T=64, control=True)


def test_backward_cfg3_shape_straddling(ops):
    """32 x 16 x 256^2 with evolving, straddling alpha: every 8th step of T = 16, the chained T = 8 backward"""
    prm = rand_cond_prm(16, seed=65, out_scale=0.5)
    gen = torch.Generator().manual_seed(650)
    x0 = torch.rand(32, 16, 256, 256, generator=gen)
    x0[:, 3] *= 0.12
    goal = torch.randn(32, 12, 256, 256, generator=gen) * 0.5
    _backward_case(ops, "32x16x256^2 straddling", prm, x0.to(DEV), goal.to(DEV), 16,
                   Draws(ops, "uniform", 32, 256, 256, 16, 0.5, gen_seed=651), every=8, chain_T=8)


def test_backward_c32_hidden28(ops):
    """C = 32, hidden 28 (front + matrix kernels)"""
    prm = rand_cond_prm(32, seed=66, hidden=28, out_scale=1.0)
    gen = torch.Generator().manual_seed(660)
    x0 = torch.rand(2, 32, 64, 64, generator=gen)
    x0[:, 3] *= 0.12
    goal = torch.randn(2, 28, 64, 64, generator=gen) * 0.5
    _backward_case(ops, "2x32x64^2 hidden 28 straddling", prm, x0.to(DEV), goal.to(DEV), 16,
                   Draws(ops, "bits", 2, 64, 64, 16, 0.5, gen_seed=661), every=1, chain_T=16)


# ------------------------------------------------------------------------------------------------ negative controls
def test_replay_flags_a_changed_slot_and_a_flipped_mask(ops):
    prm = rand_cond_prm(20, seed=61, out_scale=1.0)
    x0, goal = _train_inputs(8, 20, 64, 610, "seed")
    dr = Draws(ops, "philox", 8, 64, 64, 64, 0.5, seed=7)
    w = _cond_w(ops, prm, x0)
    out, states, pre = ops.cond_grow(x0, 64, goal, None, w, 3, seed=dr.seed, keep_history=True)
    p64, gpad = _f64(prm), O.cond_pad_goal(goal.double(), 20)
    k = 40
    life = pre[k].bool() & ops.cond_alive(states[k], 3)[:, 0]
    live = life.nonzero()
    b, y, x = [int(v) for v in live[len(live) // 2]]
    s = states.clone()
    s[k, b, 0, y, x] += 1e-3
    worst, _, bad = _replay(s, pre, out, gpad, dr, p64, 3, 0.5, flags=True)
    nb = torch.zeros_like(bad[k])
    nb[b, 0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    elsewhere = sum(int(m.sum()) for j, m in bad.items() if j not in (k - 1, k))
    _say("negative control: slot 40 + 1e-3", flagged_at_39=int(bad[k - 1].sum()), flagged_at_40=int(bad[k].sum()),
         flagged_at_40_outside_3x3=int((bad[k] & ~nb).sum()), flagged_elsewhere=elsewhere)
    assert bool(bad[k - 1][b, 0, y, x]) and int(bad[k - 1].sum()) == 1
    assert not bool((bad[k] & ~nb).any()) and elsewhere == 0
    del s
    p = pre.clone()
    p[k + 1, b, y, x] ^= 1
    worst, _, bad = _replay(states, p, out, gpad, dr, p64, 3, 0.5, flags=True)
    _say("negative control: flipped pre byte", pre_mismatch=worst["pre"])
    assert worst["pre"] >= 1 and bool(bad[k][b, 0, y, x])
