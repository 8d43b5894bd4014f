"""Host side of the opt-in bf16-MFMA TRAINING mode of DyNCA (include/ncahip.h, "bf16-MFMA training"): the float64 restatement of the
backward contract the GPU tests (test_gpu_dynca_train_bf16.py) compare the kernels with, the stage caps they use, the exports, the
refusals and the Python plumbing -- none of which needs a GPU.

The reference.  stage_step() restates ONE backward step of the contract (perception in float64 from oracle.nca_oracle, the
roundings through .to(torch.bfloat16), every product in float64, the stencil adjoint as torch.autograd.grad of the float64
perception); contract_backward() chains it over a history.  With rb = identity it IS autograd through the oracle's float64 steps
(first test).

The stage caps (check_* below; the GPU file imports them).  Every stage is compared with a float64 evaluation FED THE KERNEL'S OWN
PREVIOUS STAGE, so each tolerance is the fp32 summation error of that stage alone (u = 2^-24, a sum of n terms evaluated in fp32 in
any order is within n * 2^-23 * sum|terms| of the exact one with room to spare) plus, where the stage ends in a bf16 rounding, one
bf16 ulp of the result on a capped share of the elements (a value whose fp32 sum sits within the summation error of a rounding
boundary may go the other way: FLIP_FRACTION of test_dynca_bf16_host.py, 0.5 %).  The last test group evaluates the same contract
in fp32 on the CPU and holds it to every cap ("the reference alone is inside"), then plants four defects that must miss them."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from test_dynca_bf16_host import FLIP_FRACTION, _rb, bf16_inputs, contract_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 0.5
U23 = 2.0 ** -23
FLAG_FRACTION = 0.001          # share of hidden units whose float64 pre-activation lies within the fp32-summation bound of zero

# (B, C, fc, c_cond, H, W, pad): the smallest shapes at which each code path of the kernels can go wrong
ROWS = {
    "a": (1, 12, 96, 3, 16, 16, "circular"),     # reference default, <12, 96>, vector form
    "b": (2, 16, 128, 2, 16, 32, "replicate"),   # <16, 128>, CPE conditioning
    "c": (1, 9, 80, 0, 6, 10, "reflect"),        # C % 4 != 0, fc % 32 != 0, no conditioning, any-shape form, partial tile
    "d": (1, 16, 128, 1, 20, 24, "constant"),    # zero padding; partial tiles on both axes
    "e": (2, 12, 96, 3, 48, 32, "circular"),     # 12 tiles: the per-workgroup partial reduction
}
MS_ROWS = {"a": ROWS["a"], "f": (1, 16, 128, 0, 10, 14, "replicate")}    # two-scale: row a, and the any-shape form
SEEDS = {"a": 11, "b": 12, "c": 13, "d": 14, "e": 15, "f": 16}
# close-to-fp32 literal: worst relative L2 distance of the contract's gradients from the exact float64 gradients of the same history,
# over every row above (single- and two-scale, T = 3), times 2 because the GPU's accumulation order differs.  Measured values: see
# test_distance_of_the_contract_from_the_exact_gradients.
CLOSE_TO_F32 = 2 * 0.082       # worst: b1 of single-scale row b, 8.18e-2


def make_case(row, two=False, T=3, device="cpu", seed=None):
    """inputs of one case row: prm, x0, cond, us [T,B,1,H,W], cotangents g_final and g_states [T+1,B,C,H,W] (slot T unused: zero)"""
    B, C, fc, cc, H, W, pad = (MS_ROWS if two else ROWS)[row]
    prm, x, cond, _ = bf16_inputs(C, fc, cc, B, H, W, seed=(SEEDS[row] + (100 if two else 0)) if seed is None else seed)
    g = torch.Generator().manual_seed(1000 + SEEDS[row])
    us = torch.rand(T, B, 1, H, W, generator=g)
    g_final = torch.randn(B, C, H, W, generator=g)
    g_states = torch.randn(T + 1, B, C, H, W, generator=g) * 0.3
    g_states[T] = 0
    mv = lambda t: None if t is None else t.to(device)             # noqa: E731
    return dict(prm={k: v.to(device) for k, v in prm.items()}, x=mv(x), cond=mv(cond), us=mv(us), g_final=mv(g_final), g_states=mv(g_states),
                pad=pad, scales=(0, 1) if two else (0,), dims=(B, C, fc, cc, H, W))


def _mats(prm, dtype):
    return (prm["w1.weight"].to(dtype)[:, :, 0, 0], prm["w1.bias"].to(dtype), prm["w2.weight"].to(dtype)[:, :, 0, 0])


def _mask(u, dtype):
    return (u.float() + torch.tensor(RATE, dtype=torch.float32)).floor().to(dtype)          # floorf(u + rate) in fp32, as the kernels


def stage_step(x, g, cond, u, prm, pad, scales=(0,), rb=_rb, dtype=torch.float64, gate_from=None, db1_from_dh=False):
    """every stage of ONE backward step of the contract, evaluated in `dtype`.  gate_from / db1_from_dh plant defects (tests below)."""
    C = x.shape[1]
    xd = x.to(dtype).detach().requires_grad_(True)
    yfull = O.dynca_perceive_multiscale(xd, pad, scales, None if cond is None else cond.to(dtype))
    y = yfull.detach()
    w1, b1, w2 = _mats(prm, dtype)
    w1b, w2b, yb = rb(w1), rb(w2), rb(y)
    a1 = torch.einsum("jk,bkhw->bjhw", w1b, yb) + b1[None, :, None, None]
    gate = (a1 if gate_from is None else gate_from) > 0
    hb = rb(F.relu(a1))
    gb = rb(g.to(dtype) * _mask(u, dtype))
    dh = torch.einsum("cj,bchw->bjhw", w2b, gb) * gate
    dhb = rb(dh)
    dy = torch.einsum("jk,bjhw->bkhw", w1b[:, :4 * C], dhb)
    (adj,) = torch.autograd.grad(yfull[:, :4 * C], xd, dy)
    return dict(y=y, yb=yb, a1=a1, hb=hb, gb=gb, dh=dh, dhb=dhb, dy=dy, adj=adj,
                w2=torch.einsum("bchw,bjhw->cj", gb, hb), b2=gb.sum((0, 2, 3)),
                w1=torch.einsum("bjhw,bkhw->jk", dhb, yb), b1=(dh if db1_from_dh else dhb).sum((0, 2, 3)))


def contract_backward(x_hist, g_final, g_states, cond, u, prm, pad, scales=(0,), rb=_rb, dtype=torch.float64, **defects):
    """dL/dx_0 and the four weight gradients of the contract over the history x_hist [T+1,...] (slots 0..T-1 are read), in `dtype`.
    u [T,B,1,H,W]; g_final = dL/dx_T including any cotangent of x_T itself; g_states (or None): slots 0..T-1 are added where
    x_t's gradient is formed, as the drivers do."""
    T = u.shape[0]
    g = g_final.to(dtype)
    acc = None
    for t in range(T - 1, -1, -1):
        s = stage_step(x_hist[t], g, cond, u[t], prm, pad, scales, rb, dtype, **defects)
        g = g + s["adj"] + (0 if g_states is None else g_states[t].to(dtype))
        acc = {k: s[k] + (0 if acc is None else acc[k]) for k in ("w1", "b1", "w2", "b2")}
    return dict(x0=g, **acc)


def exact_history(c, T, dtype=torch.float64):
    """the oracle's trajectory [T+1,...] in `dtype`"""
    cond = None if c["cond"] is None else c["cond"].to(dtype)
    p = {k: v.to(dtype) for k, v in c["prm"].items()}
    xs = [c["x"].to(dtype)]
    for t in range(T):
        xs.append(O.dynca_step(xs[-1], cond, c["us"][t].to(dtype), p, c["pad"], RATE, c["scales"]))
    return torch.stack(xs)


def contract_history(c, T):
    """the mode-1 forward trajectory of the contract (float64 evaluation of test_dynca_bf16_host.contract_step), rounded to fp32 slots"""
    xs = [c["x"]]
    for t in range(T):
        xs.append(contract_step(xs[-1], c["cond"], c["us"][t], c["prm"], c["pad"], RATE, c["scales"])[0].float())
    return torch.stack(xs)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ------------------------------------------------------------------ the reference is autograd where nothing is rounded
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("two", [False, True], ids=["single", "two_scale"])
@pytest.mark.parametrize("row", ["a", "f_or_c"])
def test_identity_rounding_is_autograd_through_the_oracle(row, two, T):
    """rb = identity: contract_backward equals torch autograd through the oracle's float64 steps to 1e-12 (with / without cond)"""
    row = row if row == "a" else ("f" if two else "c")
    c = make_case(row, two, T)
    x0 = c["x"].double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in c["prm"].items()}
    cond = None if c["cond"] is None else c["cond"].double()
    xs, loss = [x0], 0
    for t in range(T):
        loss = loss + (xs[-1] * c["g_states"][t].double()).sum()
        xs.append(O.dynca_step(xs[-1], cond, c["us"][t].double(), p, c["pad"], RATE, c["scales"]))
    loss = loss + (xs[-1] * c["g_final"].double()).sum()
    ref = torch.autograd.grad(loss, [x0, p["w1.weight"], p["w1.bias"], p["w2.weight"], p["w2.bias"]])
    got = contract_backward(torch.stack([x.detach() for x in xs]), c["g_final"], c["g_states"], c["cond"], c["us"], c["prm"], c["pad"],
                            c["scales"], rb=lambda t: t)
    for k, r in zip(("x0", "w1", "b1", "w2", "b2"), ref):
        e = rel_l2(got[k], r.reshape(got[k].shape))
        print(f"row {row} two_scale={two} T={T} {k}: {e:.2e}")
        assert e < 1e-12, (k, e)


# ------------------------------------------------------------------ the stage caps
def bf16_ulp(v):
    """one unit in the last place of bf16 at |v| (8 significant bits); the smallest normal's for zero"""
    return torch.exp2(torch.floor(torch.log2(v.abs().double().clamp_min(2.0 ** -126))) - 7)


def from_bits(t):
    """bf16 bit patterns (int16 / bfloat16 tensor) -> float64 values"""
    return (t.view(torch.bfloat16) if t.dtype == torch.int16 else t).double()


def _abs_perceive(x, pad, scale=0):
    """the perception with |filters| on |x|: sum of |terms| of every perception value; scale 1: between the two bilinear resamplings of
    oracle.dynca_perceive, whose weights are positive"""
    if scale:
        h, w = x.shape[2:]
        down = F.interpolate(x.abs(), size=(h // 2, w // 2), mode="bilinear", align_corners=False)
        return F.interpolate(_abs_perceive(down, pad), size=(h, w), mode="bilinear", align_corners=False)
    xa = x.abs()
    ab = lambda f: [[abs(v) for v in r] for r in f]               # noqa: E731
    return torch.cat([xa, O._depthwise_fixed(xa, ab(O.SOBEL_X), pad), O._depthwise_fixed(xa, ab([list(r) for r in zip(*O.SOBEL_X)]), pad),
                      O._depthwise_fixed(xa, ab(O.LAPLACIAN), pad)], dim=1)


def _ulp_stage(got, ref, slack, skip, what):
    """got within one bf16 ulp (+ slack: the fp32 summation error of the value that is rounded) of ref, equal on all but FLIP_FRACTION;
    elements in `skip` are not compared.  Prints first."""
    d = (got - ref).abs()
    keep = ~skip if skip is not None else torch.ones_like(d, dtype=torch.bool)
    over = float(((d - slack) / bf16_ulp(torch.maximum(ref.abs(), got.abs())))[keep].max())
    differ = float(((d > slack) & keep).double().sum() / keep.double().sum())
    print(f"{what}: worst (|d| - slack) / ulp {over:.3f} (cap 1), differing share {100 * differ:.3f} % (cap {100 * FLIP_FRACTION:g} %), "
          f"skipped {0 if skip is None else int(skip.sum())}")
    assert over <= 1.0, (what, over)
    assert differ <= FLIP_FRACTION, (what, differ)


def check_y(y_got, x, pad, what="y_out"):
    """y_out (values of the kernel's bf16) against rb(float64 perception): one ulp, equal on all but FLIP_FRACTION.  slack: the fp32
    evaluation of a perception value (9 taps) is within 16 * 2^-24 * sum|taps| of the float64 one."""
    x64 = x.double()
    ref = _rb(O.dynca_perceive(x64, pad))
    _ulp_stage(y_got.double(), ref, 2.0 ** -20 * _abs_perceive(x64, pad), None, what)


def check_dh(dh_got, y_got, g, cond, u, prm, what="dh_out"):
    """dh_out against rb(ref dh) computed in float64 FROM THE KERNEL'S y_out.  Hidden units whose float64 a1 lies within the fp32
    summation bound K1 * 2^-23 * sum|terms| of zero are flagged and skipped (their gate may go either way); at most FLAG_FRACTION."""
    w1, b1, w2 = _mats(prm, torch.float64)
    w1b, w2b = _rb(w1), _rb(w2)
    yb = y_got.double() if cond is None else torch.cat([y_got.double(), _rb(cond.double())], dim=1)
    a1 = torch.einsum("jk,bkhw->bjhw", w1b, yb) + b1[None, :, None, None]
    terms = torch.einsum("jk,bkhw->bjhw", w1b.abs(), yb.abs()) + b1.abs()[None, :, None, None]
    flagged = a1.abs() <= (w1.shape[1] + 1) * U23 * terms
    share = float(flagged.double().mean())
    print(f"{what}: flagged share {100 * share:.4f} % (cap {100 * FLAG_FRACTION:g} %)")
    assert share <= FLAG_FRACTION, (what, share)
    gb = _rb(g.double() * _mask(u, torch.float64))
    ref = _rb(torch.einsum("cj,bchw->bjhw", w2b, gb) * (a1 > 0))
    slack = w2.shape[0] * U23 * torch.einsum("cj,bchw->bjhw", w2b.abs(), gb.abs())
    _ulp_stage(dh_got.double(), ref, slack, flagged, what)
    return dict(a1=a1, gb=gb, hb=_rb(F.relu(a1)), flagged=flagged, delta=(w1.shape[1] + 1) * U23 * terms)


def _sum_stage(got, ref, bound, what):
    d = (got.double() - ref).abs()
    worst = float((d / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    off = float(d[bound <= 0].max()) if bool((bound <= 0).any()) else 0.0
    print(f"{what}: worst |d| / bound {worst:.3e}, where the bound is 0: {off:.1e}, max |ref| {float(ref.abs().max()):.3g}")
    assert bool((d <= bound).all()), (what, worst, off)


def check_dy(dy_got, dh_got, prm, C, what="dL/dy"):
    """dL/dy against the float64 product of the kernel's dh_out: within fc * 2^-23 * sum_j |w1b_jk dhb_j| per element"""
    w1b = _rb(prm["w1.weight"].double()[:, :4 * C, 0, 0])
    ref = torch.einsum("jk,bjhw->bkhw", w1b, dh_got.double())
    bound = w1b.shape[0] * U23 * torch.einsum("jk,bjhw->bkhw", w1b.abs(), dh_got.double().abs())
    _sum_stage(dy_got, ref, bound, what)
    return ref, bound


def check_gram(out_got, a, b, what="gram"):
    """[a b^T | row sums of a] over all cells against float64 products of the same bf16 values: within n * 2^-23 * sum|a b|"""
    a, b = a.double(), b.double()
    n, ma, nb = a.shape[0] * a.shape[2] * a.shape[3], a.shape[1], b.shape[1]
    ref = torch.cat([torch.einsum("bihw,bjhw->ij", a, b).reshape(-1), a.sum((0, 2, 3))])
    bound = n * U23 * torch.cat([torch.einsum("bihw,bjhw->ij", a.abs(), b.abs()).reshape(-1), a.abs().sum((0, 2, 3))])
    assert out_got.numel() == ma * nb + ma
    _sum_stage(out_got.reshape(-1), ref, bound, what)


def check_gw2(gw2_got, st, what="gw2_out"):
    """gw2_out = [gb hb^T | sum gb] against float64 products of gb and of hb = rb(relu(a1)) recomputed from the kernel's y_out (st:
    check_dh's return): within n * 2^-23 * sum|gb hb|.  The kernel does not write hb, so the reference's hb is not the kernel's own
    value where the kernel's fp32 a1 (within delta = the summation bound of the float64 a1) falls on the other side of a bf16 rounding
    boundary: exactly the elements whose relu(a1) lies within delta of a midpoint between two bf16 values (hb one ulp away) or within
    delta of zero (hb anywhere in [0, bf16(delta)]).  Their exact worst contribution, sum|gb| * that uncertainty, is added; every other
    element contributes nothing beyond the summation term."""
    gb, hb, a1, delta = st["gb"], st["hb"], st["a1"], st["delta"]
    n = gb.shape[0] * gb.shape[2] * gb.shape[3]
    v = F.relu(a1)
    ulp = bf16_ulp(v)
    frac = v / ulp - torch.floor(v / ulp)                           # position between the two neighbouring bf16 values
    near_mid = ((frac - 0.5).abs() * ulp <= delta) & (v > delta)
    near_zero = a1.abs() <= delta
    unc = torch.where(near_zero, 2 * delta + bf16_ulp(2 * delta), torch.where(near_mid, bf16_ulp(v + delta), torch.zeros_like(v)))
    print(f"{what}: hb uncertain on {int(near_mid.sum())} elements near a rounding midpoint and {int(near_zero.sum())} near zero, of {v.numel()}")
    prod = torch.einsum("bchw,bjhw->cj", gb.abs(), hb.abs())
    extra = torch.einsum("bchw,bjhw->cj", gb.abs(), unc)
    ref = torch.cat([torch.einsum("bchw,bjhw->cj", gb, hb).reshape(-1), gb.sum((0, 2, 3))])
    bound = torch.cat([(n * U23 * prod + extra).reshape(-1), n * U23 * gb.abs().sum((0, 2, 3))])
    _sum_stage(gw2_got.reshape(-1), ref, bound, what)


def check_gx(gx_got, g, dy_ref, dy_bound, x, pad, what="g_x"):
    """g_x against g + stencil-adjoint(dy_ref) in float64 (dy_ref, dy_bound: check_dy's return): within the adjoint's absolute-value
    propagation of the dL/dy bound, plus the fp32 evaluation of the adjoint itself (16 * 2^-24 of its sum of |terms|)"""
    def adj(v, absolute):
        xd = x.double().detach().requires_grad_(True)
        (r,) = torch.autograd.grad(_abs_perceive(xd, pad) if absolute else O.dynca_perceive(xd, pad), xd, v)
        return r
    # _abs_perceive takes |x| first: its derivative carries sign(x); the propagation wanted is the one of the |filters| alone
    def adj_abs(v):
        xd = torch.ones_like(x, dtype=torch.float64).requires_grad_(True)
        (r,) = torch.autograd.grad(_abs_perceive(xd, pad), xd, v)
        return r
    ref = g.double() + adj(dy_ref, False)
    bound = adj_abs(dy_bound) + 2.0 ** -20 * (g.double().abs() + adj_abs(dy_ref.abs()))
    _sum_stage(gx_got, ref, bound, what)


def run_stage_checks(got, c, t=0, x=None, g=None):
    """all stage caps on one step's outputs: got = dict y, dh (values of the bf16 buffers), dy, gx, gw2, gram (fp32).  c: make_case"""
    B, C, fc, cc, H, W = c["dims"]
    x = c["x"] if x is None else x
    g = c["g_final"] if g is None else g
    check_y(got["y"], x, c["pad"])
    st = check_dh(got["dh"], got["y"], g, c["cond"], c["us"][t], c["prm"])
    dy_ref, dy_bound = check_dy(got["dy"], got["dh"], c["prm"], C)
    check_gw2(got["gw2"], st)
    b = got["y"] if c["cond"] is None else torch.cat([got["y"].double(), _rb(c["cond"].double())], dim=1)
    check_gram(got["gram"], got["dh"], b)
    check_gx(got["gx"], g, dy_ref, dy_bound, x, c["pad"])


ROUND_L2 = 3 * 2.0 ** -8 * FLIP_FRACTION ** 0.5 + 1e-5


def t1_reference(c):
    """One backward step (T = 1, single- or two-scale) of case c in float64, and what an honest fp32 implementation may differ by.
    Returns (ref, G): ref = contract_backward's five gradients; G[k] = an elementwise bound on the effect of the gates that are not
    determined at fp32 precision.  A hidden unit is undetermined when its float64 |a1| is at most
        delta = (K1 + 1) 2^-23 sum|terms|  +  sum_k |w1b_jk| uy_k ,
    the fp32 summation bound plus the effect of every yb_k that may round the other way (uy_k = one bf16 ulp where the float64 y_k
    lies within the fp32 evaluation error 2^-19 sum|taps| of a rounding midpoint, else 0).  Such a unit's dh is either 0 or its full
    value, every gradient is linear in dhb, so the deviation is at most the absolute-value propagation of those full values: G.  At
    T = 1 nothing amplifies.  What remains are the one-ulp rounding flips of yb, hb and dhb, on at most FLIP_FRACTION of the elements
    each (the stage caps): relative L2 3 * 2^-8 * sqrt(FLIP_FRACTION), and fp32 summation (1e-5): ROUND_L2 = 8.4e-4.  A tensor passes when
        |got - ref|_2 <= |G_k|_2 + ROUND_L2 |ref_k|_2 ."""
    B, C, fc, cc, H, W = c["dims"]
    x, pad, scales = c["x"].double(), c["pad"], c["scales"]
    cond = None if c["cond"] is None else c["cond"].double()
    y = O.dynca_perceive_multiscale(x, pad, scales, cond)
    yabs = sum(_abs_perceive(x, pad, s) for s in scales) / len(scales)
    ey = 2.0 ** -19 * (yabs if cond is None else torch.cat([yabs, torch.zeros_like(cond)], dim=1))
    ulp = bf16_ulp(y)
    frac = y.abs() / ulp - torch.floor(y.abs() / ulp)
    uy = torch.where((frac - 0.5).abs() * ulp <= ey, 2 * ulp, torch.zeros_like(y))
    w1, b1, w2 = _mats(c["prm"], torch.float64)
    w1b, w2b, yb = _rb(w1), _rb(w2), _rb(y)
    a1 = torch.einsum("jk,bkhw->bjhw", w1b, yb) + b1[None, :, None, None]
    terms = torch.einsum("jk,bkhw->bjhw", w1b.abs(), yb.abs()) + b1.abs()[None, :, None, None]
    und = a1.abs() <= (w1.shape[1] + 1) * U23 * terms + torch.einsum("jk,bkhw->bjhw", w1b.abs(), uy)
    gb = _rb(c["g_final"].double() * _mask(c["us"][0], torch.float64))
    D = torch.einsum("cj,bchw->bjhw", w2b, gb).abs() * und * (1 + 2.0 ** -7)
    Gdy = torch.einsum("jk,bjhw->bkhw", w1b[:, :4 * C].abs(), D)
    ones = torch.ones_like(x).requires_grad_(True)
    (Gx,) = torch.autograd.grad(sum(_abs_perceive(ones, pad, s) for s in scales) / len(scales), ones, Gdy)
    G = dict(x0=Gx, w1=torch.einsum("bjhw,bkhw->jk", D, yb.abs() + uy), b1=D.sum((0, 2, 3)), w2=torch.zeros(C, fc, dtype=torch.float64, device=x.device),
             b2=torch.zeros(C, dtype=torch.float64, device=x.device))
    ref = contract_backward(c["x"][None], c["g_final"], c["g_states"][:1], c["cond"], c["us"][:1], c["prm"], pad, scales)
    print(f"T = 1 reference: {int(und.sum())} of {und.numel()} gates undetermined at fp32 precision")
    return ref, G


def check_t1(got, c, what=""):
    """the five gradients of a T = 1 backward (g_states slot 0 included) against t1_reference; prints first"""
    ref, G = t1_reference(c)
    for k in ("x0", "w1", "b1", "w2", "b2"):
        d, n = float((got[k].double() - ref[k]).norm()), float(ref[k].norm())
        tol = float(G[k].norm()) + ROUND_L2 * n
        print(f"{what} {k}: |got - ref| / |ref| {d / n:.3e}, tolerance {tol / n:.3e} (gates {float(G[k].norm()) / n:.2e} + roundings {ROUND_L2:.2e})")
        assert d <= tol, (what, k, d / n, tol / n)


@pytest.mark.parametrize("two,row", [(True, "a"), (True, "f"), (False, "b"), (False, "c")])
def test_reference_alone_is_inside_the_t1_tolerance(two, row):
    """the contract in fp32 (CPU) against the float64 T = 1 reference; and a planted defect -- yb wrong by one ulp on 5 % of the cells,
    far below the close-to-fp32 literal -- misses it"""
    c = make_case(row, two, 1)
    run = lambda rb: contract_backward(c["x"][None], c["g_final"], c["g_states"][:1], c["cond"], c["us"][:1], c["prm"], c["pad"],   # noqa: E731
                                       c["scales"], rb=rb, dtype=torch.float32)
    check_t1(run(_rb), c, f"contract fp32 {'two' if two else 'single'} {row}")
    gen = torch.Generator().manual_seed(1)

    def bad_rb(t):                                # the perception operand (the only 4-d tensor with 4C + cc channels): +1 ulp on 5 % of its elements
        r = _rb(t)
        if t.dim() == 4 and t.shape[1] == 4 * c["dims"][1] + c["dims"][3]:
            r = torch.where(torch.rand(t.shape, generator=gen) < 0.05, r * (1 + 2.0 ** -7), r)
        return r
    with pytest.raises(AssertionError):
        check_t1(run(bad_rb), c, "planted: yb off by one ulp on 5 %")


def cpu_stage_outputs(c, rb=_rb, **defects):
    """what the kernels write for step 0 of a case, evaluated by the contract in fp32 on the CPU (the kernels' precision)"""
    s = stage_step(c["x"], c["g_final"], c["cond"], c["us"][0], c["prm"], c["pad"], (0,), rb, torch.float32, **defects)
    C = c["dims"][1]
    return dict(y=s["yb"][:, :4 * C], dh=s["dhb"], dy=s["dy"], gx=c["g_final"] + s["adj"], gw2=torch.cat([s["w2"].reshape(-1), s["b2"]]),
                gram=torch.cat([s["w1"].reshape(-1), s["b1"]]))


@pytest.mark.parametrize("row", sorted(ROWS))
def test_reference_alone_is_inside_every_stage_cap(row):
    """the contract in fp32 (CPU) against the float64 stage references, every GPU case row and its seed; the flagged share of the
    chosen seeds stays below FLAG_FRACTION (asserted inside check_dh)"""
    c = make_case(row)
    run_stage_checks(cpu_stage_outputs(c), c)


def test_stage_caps_catch_planted_defects():
    """truncation instead of RNE on dhb; a dropped k chunk in W1b^T dhb; the gate from an exact-fp32 a1; db1 from unrounded dh"""
    c = make_case("e")
    C = c["dims"][1]
    good = cpu_stage_outputs(c)
    trunc = lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)         # noqa: E731
    # 1. truncation of dhb only: everything else rounded to nearest
    s = stage_step(c["x"], c["g_final"], c["cond"], c["us"][0], c["prm"], c["pad"], dtype=torch.float32)
    bad = dict(good, dh=trunc(s["dh"]))
    with pytest.raises(AssertionError):
        check_dh(bad["dh"], bad["y"], c["g_final"], c["cond"], c["us"][0], c["prm"], "truncated dhb")
    # 2. W1b^T dhb without its last 32 hidden units
    w1b = _rb(c["prm"]["w1.weight"][:, :4 * C, 0, 0]).clone()
    w1b[-32:] = 0
    with pytest.raises(AssertionError):
        check_dy(torch.einsum("jk,bjhw->bkhw", w1b, good["dh"]), good["dh"], c["prm"], C, "dropped k chunk")
    # 3. the gate of the exact fp32 pre-activation (unrounded operands) instead of the contract's a1
    w1, b1, _ = _mats(c["prm"], torch.float32)
    y = O.dynca_perceive_multiscale(c["x"], c["pad"], (0,), c["cond"])
    exact_a1 = torch.einsum("jk,bkhw->bjhw", w1, y) + b1[None, :, None, None]
    bad = cpu_stage_outputs(c, gate_from=exact_a1)
    with pytest.raises(AssertionError):
        check_dh(bad["dh"], bad["y"], c["g_final"], c["cond"], c["us"][0], c["prm"], "exact-fp32 gate")
    # 4. db1 from the unrounded dh, on a case where that differs by more than the cap: the roundings add up like sqrt(n) * 2^-9, the cap
    #    grows like n * 2^-23 per summed element, so the defect shows at the small rows (n = 256 here), not at n = 3072
    c = make_case("a")
    C = c["dims"][1]
    good = cpu_stage_outputs(c)
    bad = cpu_stage_outputs(c, db1_from_dh=True)
    fc, k1 = c["dims"][2], 4 * C + c["dims"][3]
    assert float((bad["gram"][fc * k1:] - good["gram"][fc * k1:]).abs().max()) > 0
    b = torch.cat([good["y"], _rb(c["cond"])], dim=1)
    with pytest.raises(AssertionError):
        check_gram(bad["gram"], good["dh"], b, "db1 from unrounded dh")


@pytest.mark.parametrize("two,row", [(False, r) for r in sorted(ROWS)] + [(True, r) for r in sorted(MS_ROWS)])
def test_distance_of_the_contract_from_the_exact_gradients(two, row):
    """relative L2 distance, per gradient tensor, of the contract's gradients (mode-1 history) from the exact float64 gradients of
    the SAME history, T = 3 with g_states.  CLOSE_TO_F32 is twice the worst.  These weight distributions are expansive (|x| grows ~10x
    per step), so a gate that the operand roundings flip -- the contract's gate is the one of ITS a1 -- carries weight: the distances
    are percents, not the 2^-8 of one rounding.  Measured (x0 / w1 / b1 / w2 / b2):
        single a 2.98e-2 2.39e-2 4.06e-2 1.42e-2 2.56e-2      b 7.00e-2 6.17e-2 8.18e-2 3.61e-2 4.52e-2
        single c 1.58e-2 1.72e-2 2.19e-2 1.54e-2 2.47e-2      d 4.36e-2 3.93e-2 4.64e-2 2.63e-2 3.12e-2
        single e 6.46e-2 5.40e-2 7.45e-2 2.98e-2 6.61e-2
        two    a 4.85e-2 4.08e-2 4.10e-2 2.87e-2 3.08e-2      f 5.44e-2 4.32e-2 6.96e-2 1.96e-2 3.24e-2"""
    c = make_case(row, two)
    hist = contract_history(c, 3)
    got = contract_backward(hist, c["g_final"], c["g_states"], c["cond"], c["us"], c["prm"], c["pad"], c["scales"])
    ref = contract_backward(hist, c["g_final"], c["g_states"], c["cond"], c["us"], c["prm"], c["pad"], c["scales"], rb=lambda t: t)
    e = {k: rel_l2(got[k], ref[k]) for k in ("x0", "w1", "b1", "w2", "b2")}
    print(f"{'two' if two else 'single'} {row}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) * 2 <= CLOSE_TO_F32, e
    assert max(e.values()) > 1e-4            # the mode does round: the literal is not vacuous


# ------------------------------------------------------------------ exports, refusals, workspace queries
NEW = ["ncahip_dynca_step_bwd_bfmma_f32", "ncahip_dynca_step_bwd_bfmma_workspace", "ncahip_gram_rows_bf16", "ncahip_gram_rows_bf16_workspace",
       "ncahip_dynca_nsteps_bwd_bfmma_f32", "ncahip_dynca_nsteps_bwd_bfmma_workspace", "ncahip_dynca_nsteps_bwd_ms_bfmma_f32",
       "ncahip_dynca_nsteps_bwd_ms_bfmma_workspace"]


def test_exports_are_in_header_library_and_binding():
    from ncahip import _capi
    header = open(os.path.join(ROOT, "include", "ncahip.h")).read()
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"^(int|size_t)\s+" + name + r"\s*\(", header, re.M), name
        assert name in _capi.SIGNATURES and hasattr(dll, name), name
        if name.endswith("_workspace"):
            assert _capi.RESTYPES[name] is ctypes.c_size_t if hasattr(_capi, "RESTYPES") else getattr(_capi.lib(), name).restype is ctypes.c_size_t
    assert _capi.version() == 300
    assert "mode-1 history" in header.lower() or "MODE-1 history" in header


def _nsteps_args(fn_ms, T=1, B=1, C=12, H=16, W=16, fc=96, cc=0, pad=1, ptr=0x1000, ws=0x10000, nbytes=1 << 30, rate=0.5, seed=0, **null):
    """argument tuple of the nsteps drivers with dummy (never dereferenced) pointers; null: names to pass as NULL"""
    P = lambda n: None if null.get(n) else ptr                      # noqa: E731
    return (P("states"), T, None if cc == 0 else ptr, ptr, ptr, ptr, ptr, ptr, B, C, H, W, fc, cc, pad, rate, seed, 0, P("g_final"), None,
            None if null.get("g_x0") else 0x5000, ptr, ptr, ptr, ptr, None if null.get("workspace") else ws, nbytes, None)


@pytest.mark.parametrize("ms", [False, True], ids=["single", "two_scale"])
def test_driver_refusals_before_any_launch(ms):
    from ncahip import _capi
    L = _capi.lib()
    fn = L.ncahip_dynca_nsteps_bwd_ms_bfmma_f32 if ms else L.ncahip_dynca_nsteps_bwd_bfmma_f32
    wsq = L.ncahip_dynca_nsteps_bwd_ms_bfmma_workspace if ms else L.ncahip_dynca_nsteps_bwd_bfmma_workspace
    msg = lambda: L.ncahip_last_error().decode()                    # noqa: E731
    for null in ("states", "g_final", "g_x0", "workspace"):
        assert fn(*_nsteps_args(ms, **{null: True})) == _capi.EINVAL and msg(), null
    assert fn(*_nsteps_args(ms, T=0)) == _capi.EINVAL and "T < 1" in msg()
    assert fn(*_nsteps_args(ms, C=20)) == _capi.ERANGE and msg()
    assert fn(*_nsteps_args(ms, fc=256)) == _capi.ERANGE and msg()
    need = wsq(1, 12, 16, 16, 96, 0)
    assert need > 0
    assert fn(*_nsteps_args(ms, nbytes=need - 1)) == _capi.EINVAL and "workspace too small" in msg()
    assert fn(*_nsteps_args(ms, ws=0x10004)) == _capi.ERANGE and "aligned" in msg()
    if ms:
        assert fn(*_nsteps_args(ms, H=15)) == _capi.ERANGE and "even" in msg()
        assert fn(*_nsteps_args(ms, H=2, W=16, pad=3)) == _capi.EINVAL and "reflect" in msg()
    # an attached direction field (host-only state): refused as by every backward
    assert L.ncahip_dynca_direction(0x2000, 1, 16, 16) == 0
    try:
        assert fn(*_nsteps_args(ms)) == _capi.EINVAL and "direction field" in msg()
    finally:
        assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0


def test_stage_entry_refusals_before_any_launch():
    from ncahip import _capi
    L = _capi.lib()
    msg = lambda: L.ncahip_last_error().decode()                    # noqa: E731
    p = 0x1000

    def step(C=12, fc=96, nbytes=1 << 30, ws=0x10000, y=p, g_next=p, g_x=0x3000):
        return L.ncahip_dynca_step_bwd_bfmma_f32(p, None, p, p, p, p, p, 1, C, 16, 16, fc, 0, 1, 0.5, 0, 0, g_next, g_x, y, p, p, p, 0, ws, nbytes, None)
    assert step(y=None) == _capi.EINVAL and "null" in msg()
    assert step(g_next=None) == _capi.EINVAL
    assert step(ws=None) == _capi.EINVAL
    assert step(C=20) == _capi.ERANGE and "C=20" in msg()
    assert step(fc=256) == _capi.ERANGE
    assert step(nbytes=L.ncahip_dynca_step_bwd_bfmma_workspace(1, 12, 16, 16, 96) - 1) == _capi.EINVAL and "workspace too small" in msg()
    assert step(ws=0x10002) == _capi.ERANGE and "misaligned" in msg()
    assert step(g_x=p) == _capi.EINVAL and "alias" in msg()
    assert L.ncahip_dynca_direction(0x2000, 1, 16, 16) == 0
    try:
        assert step() == _capi.EINVAL and "direction field" in msg()
    finally:
        assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0

    def gram(a=p, ma=96, nb1=48, b2=p, nb2=3, out=p, ws=0x10000, nbytes=1 << 30):
        return L.ncahip_gram_rows_bf16(a, ma, p, nb1, b2, nb2, 1, 256, out, 0, ws, nbytes, None)
    assert gram(a=None) == _capi.EINVAL and gram(out=None) == _capi.EINVAL and gram(ws=None) == _capi.EINVAL
    assert gram(b2=None) == _capi.EINVAL                             # nb2 > 0 without its tensor
    assert gram(ma=129) == _capi.ERANGE and gram(nb1=80) == _capi.ERANGE
    assert gram(nbytes=L.ncahip_gram_rows_bf16_workspace(96, 51, 1, 256) - 1) == _capi.EINVAL and "workspace too small" in msg()
    assert gram(ws=0x10002) == _capi.ERANGE


def test_workspace_queries_are_host_arithmetic():
    """0 for uncovered shapes, positive and monotone in B for covered ones; no device is touched"""
    from ncahip import _capi
    L = _capi.lib()
    for q in (L.ncahip_dynca_nsteps_bwd_bfmma_workspace, L.ncahip_dynca_nsteps_bwd_ms_bfmma_workspace):
        assert q(1, 20, 16, 16, 96, 3) == 0 and q(1, 12, 16, 16, 256, 3) == 0 and q(0, 12, 16, 16, 96, 3) == 0
        sizes = [q(B, 12, 64, 64, 96, 3) for B in (1, 2, 4, 8, 64)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    assert L.ncahip_dynca_step_bwd_bfmma_workspace(1, 20, 16, 16, 96) == 0 and L.ncahip_dynca_step_bwd_bfmma_workspace(1, 16, 16, 16, 129) == 0
    s = [L.ncahip_dynca_step_bwd_bfmma_workspace(B, 16, 64, 64, 128) for B in (1, 2, 4, 8)]
    assert s[0] > 0 and s == sorted(s), s
    assert L.ncahip_gram_rows_bf16_workspace(129, 51, 1, 256) == 0 and L.ncahip_gram_rows_bf16_workspace(96, 80, 1, 256) == 0
    s = [L.ncahip_gram_rows_bf16_workspace(128, 67, B, 4096) for B in (1, 2, 4, 8)]
    assert s[0] > 0 and s == sorted(s), s
    # the mode's scratch is smaller than the exact backward's: y and dh are bf16
    assert L.ncahip_dynca_nsteps_bwd_bfmma_workspace(8, 16, 256, 256, 128, 3) < L.ncahip_dynca_nsteps_bwd_workspace(8, 16, 256, 256, 128, 3)


# ------------------------------------------------------------------ precedence: two faults in one call
# The single-fault refusals above do not see the ORDER of the checks.  Every case below plants two faults in one call of a backward entry
# point (dummy pointers, refused on the host: nothing is dereferenced or launched) and expects the code and the whole message of the
# check that comes first.  The literals were recorded from the library before the entry points were given one body per stage; they
# hold the merged bodies to the order every entry point had.  test_dynca_train_bf16_wide_host.py (the wide range) and
# test_dynca_step_bwd_host.py (the two exact stage entries) use the same caller.
BITS = 0x5354494255                      # NCAHIP_SEED_U_IS_BITS with update_rate = 1.0: the bit-packed masks' refusal
SHORT = dict(nbytes=16)                  # a workspace far below every query's figure


def _step_args(entry, C=12, fc=96, H=16, W=16, rate=0.5, seed=0, g_next=0x1000, g_x=0x3000, ws=0x10000, nbytes=1 << 30):
    """argument tuple of a single-step stage entry (dummy pointers); the entries differ in their own outputs behind g_x"""
    p = 0x1000
    own = {"ncahip_dynca_step_bwd_f32": (p, p, p, None), "ncahip_dynca_step_bwd_w2_f32": (p, p, p, 0, ws, nbytes, None)}
    return (p, None, p, p, p, p, p, 1, C, H, W, fc, 0, 1, rate, seed, 0, g_next, g_x) + own.get(entry, (p, p, p, p, 0, ws, nbytes, None))


def _gram_args(a=0x1000, ma=96, nb1=48, nb2=3, HW=256, ws=0x10000, nbytes=1 << 30):
    return (a, ma, 0x1000, nb1, 0x1000, nb2, 1, HW, 0x1000, 0, ws, nbytes, None)


def refusal(entry, direction=False, **kw):
    """(code, message) of one refused call of a backward entry point; direction: with a direction field attached"""
    from ncahip import _capi
    L = _capi.lib()
    args = _gram_args(**kw) if "gram" in entry else _step_args(entry, **kw) if "_step_" in entry else _nsteps_args(None, **kw)
    if direction:
        assert L.ncahip_dynca_direction(0x2000, 1, 16, 16) == 0
    try:
        return getattr(L, entry)(*args), L.ncahip_last_error().decode()
    finally:
        assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0


def check_two_faults(entry, faults, call, want):
    got = refusal(entry, **call)
    print(f"{entry} [{faults}]: {got}")
    assert got == want, (entry, faults, got, want)


TWO_FAULTS = [
    ('ncahip_dynca_nsteps_bwd_f32', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_f32', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_f32', 'T0+range', dict(T=0, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_f32', 'range+alias', dict(ptr=0x5000, C=33),
     (-2, 'dynca step: C=33 fc=96 c_cond=0 exceeds (32,1024,4)')),
    ('ncahip_dynca_nsteps_bwd_f32', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_f32', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_f32', '4GiB+range', dict(H=4096, W=4096, C=33),
     (-2, 'dynca step: C=33 fc=96 c_cond=0 exceeds (32,1024,4)')),
    ('ncahip_dynca_nsteps_bwd_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'T0+range', dict(T=0, C=20),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'range+alias', dict(ptr=0x5000, C=20),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', '4GiB+range', dict(H=4096, W=4096, C=20),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'oddW+short', dict(W=15, nbytes=16),
     (-2, 'dynca two-scale step: H and W must be even (the x2 resampling is then the exact 2x2 mean / (0.25, 0.75) blend)')),
    ('ncahip_dynca_nsteps_bwd_ms_f32', 'C20+oddW', dict(C=20, W=15),
     (-2, 'dynca two-scale step: H and W must be even (the x2 resampling is then the exact 2x2 mean / (0.25, 0.75) blend)')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'T0+range', dict(T=0, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'range+alias', dict(ptr=0x5000, C=33),
     (-2, 'dynca step: C=33 fc=96 c_cond=0 exceeds (32,1024,4)')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_bf16', '4GiB+range', dict(H=4096, W=4096, C=33),
     (-2, 'dynca step: C=33 fc=96 c_cond=0 exceeds (32,1024,4)')),
    ('ncahip_dynca_nsteps_bwd_bf16', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_bf16', 'unaligned_history+short', dict(ptr=0x1004, nbytes=16),
     (-2, 'dynca nsteps bwd (bf16): B*C*H*W % 4 == 0 and 8-byte aligned states required')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'T0+range', dict(T=0, C=20),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'range+alias', dict(ptr=0x5000, C=20),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', '4GiB+range', dict(H=4096, W=4096, C=20),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'T0+range', dict(T=0, C=20),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'range+alias', dict(ptr=0x5000, C=20),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', '4GiB+range', dict(H=4096, W=4096, C=20),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'oddW+short', dict(W=15, nbytes=16),
     (-2, 'dynca two-scale step: H and W must be even (the x2 resampling is then the exact 2x2 mean / (0.25, 0.75) blend)')),
    ('ncahip_dynca_nsteps_bwd_ms_bfmma_f32', 'range+oddW', dict(C=20, W=15),
     (-2, "dynca nsteps bwd (bf16 MFMA): C=20 fc=96 outside the mode's range (C <= 16, fc <= 128)")),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'direction+null', dict(direction=True, g_next=None),
     (-1, 'dynca step bwd_bfmma: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'null+C33', dict(g_next=None, C=33),
     (-1, 'dynca step bwd_bfmma: null pointer')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'range+alias', dict(g_next=0x3000, C=20),
     (-2, 'dynca step bwd_bfmma: C=20 fc=96 outside the bf16-MFMA range (C <= 16, fc <= 128)')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'alias+4GiB', dict(g_next=0x3000, H=4096, W=4096),
     (-1, 'dynca step bwd_bfmma: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'alias+short', dict(g_next=0x3000, nbytes=16),
     (-1, 'dynca step bwd_bfmma: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'short+misaligned', dict(nbytes=16, ws=0x10002),
     (-1, 'dynca step bwd_bfmma: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'misaligned', dict(ws=0x10002),
     (-2, 'dynca step bwd_bfmma: misaligned workspace (4 bytes) or bf16 output (2 bytes)')),
    ('ncahip_dynca_step_bwd_bfmma_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd_bfmma: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca step bwd_bfmma: fc*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_gram_rows_bf16', 'null+range', dict(a=None, ma=129),
     (-1, 'gram_rows_bf16: null pointer')),
    ('ncahip_gram_rows_bf16', 'size+range', dict(HW=0, ma=129),
     (-1, 'gram_rows_bf16: bad size')),
    ('ncahip_gram_rows_bf16', 'range+misaligned', dict(ws=0x10002, nb1=80),
     (-2, 'gram_rows_bf16: ma=96 nb=83 outside (<=128 x <=79)')),
    ('ncahip_gram_rows_bf16', 'misaligned+short', dict(ws=0x10002, nbytes=16),
     (-2, 'gram_rows_bf16: misaligned pointer (bf16: 2 bytes; fp32 and workspace: 4 bytes)')),
]


@pytest.mark.parametrize("entry,faults,call,want", TWO_FAULTS, ids=[f"{e[7:]}-{f}" for e, f, _, _ in TWO_FAULTS])
def test_the_first_of_two_faults_is_reported(entry, faults, call, want):
    check_two_faults(entry, faults, call, want)


# ------------------------------------------------------------------ Python plumbing without a device
def _model(kind="edge", C=12, fc=96):
    from ncahip.models import dynca, dynca_extra
    cpu = torch.device("cpu")
    return dynca.DyNCA(C, 3, fc_dim=fc, device=cpu) if kind == "edge" else dynca_extra.DyNCA(C, 3, fc_dim=fc, device=cpu)


@pytest.mark.parametrize("kind", ["edge", "extra"])
def test_train_precision_attribute(kind):
    m = _model(kind)
    assert m.train_precision == "f32"
    m.train_precision = "bf16"
    assert m.train_precision == "bf16"
    for bad in ("fp16", "BF16", None, 1):
        with pytest.raises(ValueError):
            m.train_precision = bad
    assert m.train_precision == "bf16"          # a refused value leaves the setting


def test_autograd_records_the_effective_precision():
    """the cfg the autograd function would record: "bf16" inside the range, "f32" outside it (the setting is ignored there), and a
    bfloat16 pool together with "bf16" raises"""
    from ncahip import autograd
    seen = {}

    class _Stop(Exception):
        pass

    def fake_apply(x, cond, w1, b1, w2, b2, cfg):
        seen.update(cfg)
        raise _Stop

    real = autograd._DyncaNSteps.apply
    autograd._DyncaNSteps.apply = staticmethod(fake_apply)
    try:
        for C, fc, want, eff in [(12, 96, "bf16", "bf16"), (16, 128, "bf16", "bf16"), (12, 96, "f32", "f32"), (20, 96, "bf16", "f32"),
                                 (12, 256, "bf16", "f32")]:
            m = _model("edge", C, fc)
            m.train_precision = want
            m.mask_rng = "philox"                    # no draw: nothing here touches a device
            seen.clear()
            with pytest.raises(_Stop):
                autograd.dynca_nsteps_autograd(m, torch.zeros(1, C, 8, 8), None, 2, 0.5)
            assert seen["precision"] == eff, (C, fc, want, seen)
            assert autograd.dynca_train_precision(m, torch.zeros(1, C, 8, 8)) == eff
        m = _model("edge")
        m.train_precision = "bf16"
        m.mask_rng = "philox"
        with pytest.raises(ValueError):
            autograd.dynca_nsteps_autograd(m, torch.zeros(1, 12, 8, 8, dtype=torch.bfloat16), None, 2, 0.5)
        out_of_range = _model("edge", 20, 96)        # outside the range the setting is ignored, for a bfloat16 pool as for any other
        out_of_range.train_precision = "bf16"
        assert autograd.dynca_train_precision(out_of_range, torch.zeros(1, 20, 8, 8, dtype=torch.bfloat16)) == "f32"
        m.train_precision = "f32"                    # a bf16 pool with the default stays what it was: no refusal from this check
        assert autograd.dynca_train_precision(m, torch.zeros(1, 12, 8, 8, dtype=torch.bfloat16)) == "f32"
    finally:
        autograd._DyncaNSteps.apply = real


def test_ops_backward_refuses_an_unknown_precision_before_the_device():
    from ncahip import ops
    with pytest.raises(ValueError):
        ops.dynca_nsteps_backward(torch.zeros(2, 1, 12, 8, 8), None, None, None, torch.zeros(1, 12, 8, 8), None, 1, precision="fp16")


def test_trainer_sets_the_model_attribute():
    import inspect
    from ncahip.dynca_trainer import DyNCATrainer
    sig = inspect.signature(DyNCATrainer.__init__)
    assert sig.parameters["train_precision"].default is None
    m = _model("edge")
    m.seed_mode = "zeros"
    t = DyNCATrainer(m, lambda d: d["nca_state"].sum(), pool_size=4, size=(8, 8), batch_size=2, device=torch.device("cpu"), train_precision="bf16")
    assert t.model.train_precision == "bf16"
    with pytest.raises(ValueError):
        DyNCATrainer(m, lambda d: 0, pool_size=4, size=(8, 8), batch_size=2, device=torch.device("cpu"), train_precision="half")
    t2 = DyNCATrainer(m, lambda d: 0, pool_size=4, size=(8, 8), batch_size=2, device=torch.device("cpu"))
    assert t2.model.train_precision == "bf16"    # None: the model's own setting stays
