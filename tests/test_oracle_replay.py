"""The history replay of oracle/nca_oracle.py (cond_resolve, cond_replay_step / _forward / _vjp / _gate_region) on the CPU.

A history laid out as the kernels lay it out (include/ncahip.h, ncahip_cond_grow_fwd_f32 with ring = T + 1: slot 0 the input, slot
k the pending x'_{k-1}, pre slot k that step's pre mask) is built from the fp32 oracle's own grow.  Replayed in fp32 it must
give back every slot, mask and the final state bit for bit; in float64 every mask exactly and every value to rounding.  The
chained replay VJP must equal autograd through the oracle (G8 / G11 fixtures), the fp32 threshold must be kept in float64, and
a history changed in one element or one mask byte must be flagged where the change was made and nowhere else."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from util import T, load, near_threshold, replay_step_check, sd

F64 = torch.float64


def rand_cond_prm(C, seed, hidden=64, out_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
            "update_net.out.0.weight": torch.randn(hidden, 3 * C, 1, 1, generator=g) * (1.0 / (3 * C) ** 0.5),
            "update_net.out.0.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.2.weight": torch.randn(hidden, hidden, 1, 1, generator=g) * (1.0 / hidden ** 0.5),
            "update_net.out.2.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.4.weight": torch.randn(C, hidden, 1, 1, generator=g) * (out_scale * 0.3 / hidden ** 0.5)}


def oracle_history(x0, gpad, us, prm, alive_ch=3, thr=0.1, rate=0.5):
    """(states [T+1,B,C,H,W], pre [T+1,B,H,W] uint8, x_final) of the oracle's own grow, in the kernels' layout"""
    B, C, H, W = x0.shape
    states, pre, x = [x0], [torch.zeros(B, H, W, dtype=torch.uint8)], x0
    for u in us:
        d = O.cond_step(x, gpad, u, prm, alive_ch, thr, rate, return_all=True)
        states.append(d["x1"])
        pre.append(d["pre"][:, 0].to(torch.uint8))
        x = d["x2"]
    return torch.stack(states), torch.stack(pre), x


def g2_case(tag):
    g = load("g2_cond_grow")
    prm = sd(g)
    x0 = T(g[f"{tag}_x0"])
    return x0, O.cond_pad_goal(T(g["genc"]), x0.shape[1]), [T(u) for u in g[f"{tag}_us"]], prm, g


def straddle_case(seed=5, B=2, C=12, S=24, Tn=8):
    """random states with alpha in [0, 0.12): life masks straddle the threshold at every step"""
    gen = torch.Generator().manual_seed(seed)
    prm = rand_cond_prm(C, seed=seed, out_scale=0.5)
    x0 = torch.rand(B, C, S, S, generator=gen)
    x0[:, 3] *= 0.12
    gpad = O.cond_pad_goal(torch.randn(B, 8, S, S, generator=gen) * 0.5, C)
    us = [torch.rand(B, 1, S, S, generator=gen) for _ in range(Tn)]
    return x0, gpad, us, prm


def cases():
    x0, gpad, us, prm, _ = g2_case("seed")
    yield "g2 seed", x0, gpad, us, prm
    x0, gpad, us, prm, _ = g2_case("rand")
    yield "g2 rand", x0, gpad, us, prm
    yield ("straddle",) + straddle_case()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_fp32_replay_is_bit_exact(which):
    name, x0, gpad, us, prm = list(cases())[which]
    states, pre, xf = oracle_history(x0, gpad, us, prm)
    n = 0
    for rec in O.cond_replay_forward(states, pre, xf, gpad, us, prm, 3, dtype=torch.float32):
        if "x_final_got" in rec:
            assert torch.equal(rec["x_in"], xf), name
            n += 1
            continue
        assert torch.equal(rec["pre_ref"], rec["pre_got"]), (name, rec["k"])
        assert torch.equal(rec["pend_ref"], rec["pend_got"]), (name, rec["k"])
        n += 1
    assert n == len(us) + 1


@pytest.mark.parametrize("which", [0, 1, 2])
def test_float64_replay_matches_to_rounding(which):
    name, x0, gpad, us, prm = list(cases())[which]
    states, pre, xf = oracle_history(x0, gpad, us, prm)
    p64 = {k: v.double() for k, v in prm.items()}
    worst, near = 0.0, 0
    for rec in O.cond_replay_forward(states, pre, xf, gpad.double(), us, p64, 3):
        if "x_final_got" in rec:
            assert torch.equal(rec["x_in"], rec["x_final_got"])          # resolve is exact in float64
            continue
        bad, e = replay_step_check(rec, tol=1e-6)
        assert not bool(bad.any()), (name, rec["k"], e)
        worst = max(worst, e["fire"])
        near += int(near_threshold(rec["x_in"]).sum())
    print(f"\n[replay] {name}: float64 worst firing-cell error {worst:.3e}, near-threshold cells checked exactly {near}")
    if name == "straddle":
        assert near > 0


def _f64_history(x0, gpad, us, prm, alive_ch, thr, rate):
    states, pre, x = [x0], [torch.zeros(x0.shape[0], *x0.shape[2:], dtype=torch.uint8)], x0
    margin = float("inf")
    for u in us:
        d = O.cond_step(x, gpad, u, prm, alive_ch, thr, rate, return_all=True)
        for s in (x, d["x1"]):
            margin = min(margin, float((F.max_pool2d(s[:, alive_ch:alive_ch + 1], 3, 1, 1) - thr).abs().min()))
        states.append(d["x1"])
        pre.append(d["pre"][:, 0].to(torch.uint8))
        x = d["x2"]
    return torch.stack(states), torch.stack(pre), margin


def _vjp_against_autograd(x0, gpad, us, prm, cot, alive_ch, thr, rate):
    states, pre, margin = _f64_history(x0, gpad, us, prm, alive_ch, thr, rate)
    assert margin > 1e-6, margin          # no mask of the float64 trajectory where 0.1 and float32(0.1) could disagree
    gx, gg, gw = O.cond_replay_vjp(states, pre, gpad, us, prm, cot, alive_ch, thr, rate)
    _, rx, rg, rw = O.cond_grow_loss_grads(x0, gpad, us, prm, alive_ch, thr, rate, cot)
    errs = {"x0": gx, "goal": gg, **gw}
    refs = {"x0": rx, "goal": rg, **rw}
    for k in errs:
        e = float((errs[k] - refs[k]).abs().max() / refs[k].abs().max().clamp_min(1e-300))
        assert errs[k].dtype == F64 and e < 1e-12, (k, e)
    return states, pre


def test_replay_vjp_equals_autograd_g8():
    g = load("g8_cond_grads")
    prm = {k: v.double() for k, v in sd(g).items()}
    _vjp_against_autograd(T(g["x0"]).double(), T(g["gpad"]).double(), [T(u) for u in g["us"]], prm, T(g["cot"]).double(),
                          int(g["alive_ch"]), float(g["thr"]), float(g["fire_rate"]))


@pytest.mark.parametrize("tag", ["c20", "c32"])
def test_replay_vjp_equals_autograd_g11(tag):
    g = load("g11_cond_grads_wide")
    prm = {k[len(tag) + 4:]: T(v).double() for k, v in g.items() if k.startswith(tag + ".sd.")}
    x0 = T(g[f"{tag}.x0"]).double()
    gpad = O.cond_pad_goal(T(g[f"{tag}.goal_enc"]).double(), x0.shape[1])
    _vjp_against_autograd(x0, gpad, [T(u) for u in g[f"{tag}.us"]], prm, T(g[f"{tag}.cot"]).double(),
                          int(g[f"{tag}.alive_ch"]), float(g["thr"]), float(g["fire_rate"]))


def test_replay_vjp_one_step_form_chains():
    """cond_replay_vjp is the chain of its one-step form; its gate region is empty where no gate is near zero"""
    g = load("g8_cond_grads")
    prm = {k: v.double() for k, v in sd(g).items()}
    x0, gpad, us, cot = T(g["x0"]).double(), T(g["gpad"]).double(), [T(u) for u in g["us"]], T(g["cot"]).double()
    states, pre, _ = _f64_history(x0, gpad, us, prm, 3, 0.1, 0.5)
    seen = {}
    gx, gg, gw = O.cond_replay_vjp(states, pre, gpad, us, prm, cot, 3, on_step=lambda k, xi, gn, r: seen.__setitem__(k, (xi, gn, r)))
    assert sorted(seen) == list(range(len(us)))
    for k, (xi, gn, r) in seen.items():
        gprev = seen[k - 1][1] if k > 0 else gx
        assert torch.equal(r[0], gprev), k
        one = O.cond_replay_vjp_step(xi, states[k + 1], pre[k + 1], gpad, us[k], prm, gn, 3)
        assert torch.equal(one[0], r[0]) and torch.equal(one[1], r[1])
    region, cnt = O.cond_replay_gate_region(states, pre, gpad, us, prm, 3, 1e-6)
    ref_region, ref_cnt = O.cond_gate_influence(x0, gpad, us, prm, 3, 1e-6)
    assert torch.equal(cnt, ref_cnt) and torch.equal(region, ref_region)
    region, cnt = O.cond_replay_gate_region(states, pre, gpad, us, prm, 3, 1e-2)     # a generous margin finds gates
    ref_region, ref_cnt = O.cond_gate_influence(x0, gpad, us, prm, 3, 1e-2)
    assert int(cnt.sum()) > 0 and torch.equal(cnt, ref_cnt) and torch.equal(region, ref_region)


def test_threshold_trap():
    """pooled alpha exactly float32(0.1) is dead for the kernels (fp32 '>'), so for the replay in float64 too"""
    thr32 = float(np.float32(0.1))
    assert thr32 > 0.1
    x = torch.zeros(1, 4, 5, 5)
    x[0, 3, 2, 2] = thr32
    x[0, :3] = torch.rand(3, 5, 5, generator=torch.Generator().manual_seed(0))
    assert not bool(O.cond_alive(x, 3).any())                            # fp32 oracle, the reference's own comparison
    assert bool((F.max_pool2d(x.double()[:, 3:4], 3, 1, 1) > 0.1).any())  # the trap: a float64 '> 0.1' calls it alive
    pre = torch.ones(1, 5, 5, dtype=torch.uint8)
    assert not bool(O._alive32(x.double(), 3, 0.1).any())
    assert not bool(O.cond_resolve(x.double(), pre, 3).any())
    prm = {k: v.double() for k, v in rand_cond_prm(4, seed=1, hidden=8).items()}
    p, pend = O.cond_replay_step(x.double(), None, torch.zeros(1, 1, 5, 5), prm, 3)
    assert not bool(p.any())
    # one ulp above: alive on both sides
    x[0, 3, 2, 2] = float(np.nextafter(np.float32(0.1), np.float32(1)))
    assert bool(O._alive32(x.double(), 3, 0.1)[0, 0, 1:4, 1:4].all())
    assert torch.equal(O._alive32(x.double(), 3, 0.1), O.cond_alive(x, 3))
    # the clamp bounds and the fire rate are float32 values as well
    y = torch.rand(1, 4, 5, 5, generator=torch.Generator().manual_seed(1)) * 0.6
    y[0, 3] = 0.5
    assert torch.equal(O.cond_resolve(y.double(), pre, 3, lo=0.1, hi=0.3), O.cond_resolve(y, pre, 3, lo=0.1, hi=0.3).double())
    u = torch.full((1, 1, 5, 5), float(np.float32(0.3)))
    _, pend = O.cond_replay_step(y.double(), None, u, prm, 3, fire_rate=0.3)
    assert torch.equal(pend, y.double())                                # u == float32(0.3) does not fire at rate 0.3


def _flags(states, pre, xf, gpad, us, prm):
    p64 = {k: v.double() for k, v in prm.items()}
    out = {}
    for rec in O.cond_replay_forward(states, pre, xf, gpad.double(), us, p64, 3):
        if "x_final_got" in rec:
            out["final"] = ~(rec["x_in"] == rec["x_final_got"]).all(1, keepdim=True)
            continue
        out[rec["k"]] = replay_step_check(rec)[0]
    return out


def test_negative_controls():
    x0, gpad, us, prm = straddle_case(seed=7, Tn=8)
    states, pre, xf = oracle_history(x0, gpad, us, prm)
    clean = _flags(states, pre, xf, gpad, us, prm)
    assert not any(bool(v.any()) for v in clean.values())
    k = 4
    life = (pre[k].bool() & O.cond_alive(states[k], 3)[:, 0])
    b, y, x = [int(i) for i in life.nonzero()[len(life.nonzero()) // 2]]
    s = states.clone()
    s[k, b, 0, y, x] += 1e-3
    fl = _flags(s, pre, xf, gpad, us, prm)
    assert bool(fl[k - 1][b, 0, y, x]), "the changed slot is not flagged at the step that wrote it"
    assert int(fl[k - 1].sum()) == 1
    nb = torch.zeros_like(fl[k])
    nb[b, 0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    assert not bool((fl[k] & ~nb).any())
    assert not any(bool(v.any()) for j, v in fl.items() if j not in (k - 1, k))
    # one flipped pre byte
    p = pre.clone()
    p[k + 1, b, y, x] ^= 1
    fl = _flags(states, p, xf, gpad, us, prm)
    assert bool(fl[k][b, 0, y, x])
