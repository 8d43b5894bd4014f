"""The oracle in float64 (oracle/nca_oracle.py follows its inputs' dtype and device): the mode tests/test_gpu_fullsize_ref.py
uses as the on-device reference at full size, pinned here on the CPU against the reference-generated fp32 fixtures (G1 / G3 /
G8 / G10) and against the fp32 aten convolutions it replaces (the 1x1 layers as matrix products).  Bounds: 1e-5 relative for
outputs, 1e-4 of the largest entry for gradients -- fp32 rounding of a few steps, far below any wrong term."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from util import T, load, sd

F64 = torch.float64


def d(a):
    return T(a).double() if a.dtype != np.bool_ else T(a)


def out_err(got, ref):
    got, ref = got.detach().double(), T(ref).double() if isinstance(ref, np.ndarray) else ref.detach().double()
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


def grad_err(got, ref):
    got, ref = got.detach().double(), T(ref).double() if isinstance(ref, np.ndarray) else ref.detach().double()
    return float((got - ref).abs().max() / max(1e-12, float(ref.abs().max())))


def near_thr(x1, alive, thr, eps=2e-6):
    """cells whose pooled new alpha lies within eps of the life threshold: fp32 and float64 may resolve them differently"""
    return (F.max_pool2d(x1[:, alive:alive + 1].double(), 3, 1, 1) - thr).abs() < eps


def test_float64_keeps_dtype_everywhere():
    x = torch.rand(1, 4, 6, 7, dtype=F64)
    assert O.dynca_perceive(x, "reflect").dtype == F64
    assert O.dynca_perceive(x, "circular", scale=1).dtype == F64
    assert O.edge_extractor(x[:, :1], "tanh").dtype == F64
    assert O.cpe2d(2, 6, 7, dtype=F64).dtype == F64
    assert float((O.cpe2d(2, 6, 7, dtype=F64) - O.cpe2d(2, 6, 7).double()).abs().max()) < 1e-7
    assert O._bf(x).dtype == F64 and O._bf_ste(x).dtype == F64
    assert torch.equal(O._bf(x), O._bf(x.float()).double())


def test_conv1x1_matmul_form_matches_aten_conv():
    """the float64 1x1 layers (matrix products) against F.conv2d in float64 and in fp32"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 67, 9, 13, generator=g, dtype=F64)
    w = torch.randn(128, 67, 1, 1, generator=g, dtype=F64)
    b = torch.randn(128, generator=g, dtype=F64)
    ref = F.conv2d(x, w, b)
    assert float((O._conv1x1(x, w, b) - ref).abs().max()) < 1e-12 * float(ref.abs().max())
    assert float((O._conv1x1(x, w) - F.conv2d(x, w)).abs().max()) < 1e-12 * float(ref.abs().max())
    assert torch.equal(O._conv1x1(x.float(), w.float(), b.float()), F.conv2d(x.float(), w.float(), b.float()))
    # autograd through both forms
    xa, wa, ba = (t.clone().requires_grad_(True) for t in (x, w, b))
    xb, wb, bb = (t.clone().requires_grad_(True) for t in (x, w, b))
    cot = torch.randn(3, 128, 9, 13, generator=g, dtype=F64)
    (O._conv1x1(xa, wa, ba) * cot).sum().backward()
    (F.conv2d(xb, wb, bb) * cot).sum().backward()
    for a_, b_ in ((xa, xb), (wa, wb), (ba, bb)):
        assert grad_err(a_.grad, b_.grad) < 1e-12


def test_float64_cond_and_dynca_match_fp32_at_a_small_shape():
    """the float64 step functions against the fp32 ones (aten convolutions) on random inputs, every pad mode and both
    perception scales -- the cross-check of the matrix-product rewrite through whole steps"""
    g = torch.Generator().manual_seed(11)
    C, hid = 12, 64
    prm = {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
           "update_net.out.0.weight": torch.randn(hid, 3 * C, 1, 1, generator=g) * 0.15,
           "update_net.out.0.bias": torch.randn(hid, generator=g) * 0.1,
           "update_net.out.2.weight": torch.randn(hid, hid, 1, 1, generator=g) * 0.12,
           "update_net.out.2.bias": torch.randn(hid, generator=g) * 0.1,
           "update_net.out.4.weight": torch.randn(C, hid, 1, 1, generator=g) * 0.05}
    x = torch.rand(2, C, 14, 18, generator=g)
    x[:, 3] = 0.5 + 0.5 * x[:, 3]
    goal = torch.randn(2, C, 14, 18, generator=g) * 0.5
    u = torch.rand(2, 1, 14, 18, generator=g)
    p64 = {k: v.double() for k, v in prm.items()}
    assert out_err(O.cond_step(x.double(), goal.double(), u, p64, 3), O.cond_step(x, goal, u, prm, 3)) < 1e-5
    dp = {"w1.weight": torch.randn(96, 4 * C + 2, 1, 1, generator=g) * 0.1, "w1.bias": torch.randn(96, generator=g) * 0.1,
          "w2.weight": torch.randn(C, 96, 1, 1, generator=g) * 0.05, "w2.bias": torch.randn(C, generator=g) * 0.02}
    d64 = {k: v.double() for k, v in dp.items()}
    cond = O.cpe2d(2, 14, 18)
    for pad in O.PAD_MODES:
        for scales in ((0,), (0, 1)):
            ref = O.dynca_step(x, cond, u, dp, pad, 0.5, scales)
            got = O.dynca_step(x.double(), O.cpe2d(2, 14, 18, dtype=F64), u, d64, pad, 0.5, scales)
            assert out_err(got, ref) < 1e-5, (pad, scales)


def test_g1_cond_step_in_float64():
    g = load("g1_cond_step")
    prm = {k: v.double() for k, v in sd(g).items()}
    a, thr, rate = int(g["alive_ch"]), float(g["thr"]), float(g["fire_rate"])
    r = O.cond_step(d(g["x"]), d(g["genc"]), T(g["u"]), prm, a, thr, rate, return_all=True)
    assert r["x2"].dtype == F64
    assert torch.equal(r["pre"], T(g["pre"])) and torch.equal(r["rmask"], T(g["rmask"]))
    for k in ("p", "out", "x1"):
        assert out_err(r[k], g[k]) < 1e-5, k
    ok = ~near_thr(T(g["x1"]), a, thr).expand_as(r["x2"])
    assert float(ok.float().mean()) > 0.999
    assert out_err(r["x2"][ok], T(g["x2"])[ok]) < 1e-5


def test_g3_dynca_all_cases_in_float64():
    g = load("g3_dynca")
    cases = json.loads(str(g["cases"]))
    for c in cases:
        t = c["tag"]
        prm = {k: d(g[f"{t}.{k}"]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
        x0 = d(g[f"{t}.x0"])
        if c["cond"] == "edges":
            cond = O.edge_extractor(d(g[f"{t}.cond_img"]), c["transform"])
            assert cond.dtype == F64 and out_err(cond, g[f"{t}.cond"]) < 1e-5, c
        elif c["cond"] == "pos_emb":
            cond = O.cpe2d(*[x0.shape[i] for i in (0, 2, 3)], dtype=F64)
            assert out_err(cond, g[f"{t}.cond"]) < 1e-6, c
        else:
            cond = None
        assert out_err(O.dynca_perceive(x0, c["pad"]), g[f"{t}.perc0"]) < 1e-5, c
        xT, states = O.dynca_nsteps(x0, cond, [T(u) for u in g[f"{t}.us"]], prm, c["pad"], 0.5, collect=True)
        assert xT.dtype == F64
        assert out_err(states[0], g[f"{t}.state_first"]) < 1e-5, c
        assert out_err(states[-1], g[f"{t}.state_last"]) < 1e-5, c


def test_g8_cond_grads_in_float64():
    g = load("g8_cond_grads")
    prm = {k: v.double() for k, v in sd(g).items()}
    xT, dx0, dg, grads = O.cond_grow_loss_grads(d(g["x0"]), d(g["gpad"]), [T(u) for u in g["us"]], prm,
                                                int(g["alive_ch"]), float(g["thr"]), float(g["fire_rate"]), d(g["cot"]))
    assert xT.dtype == F64 and dx0.dtype == F64
    assert out_err(xT, g["xT"]) < 1e-5
    assert grad_err(dx0, g["d_x0"]) < 1e-4 and grad_err(dg, g["d_gpad"]) < 1e-4
    assert len(grads) == 6
    for k, v in grads.items():
        assert v.dtype == F64 and grad_err(v, g["grad." + k]) < 1e-4, k


@pytest.mark.parametrize("pad", O.PAD_MODES)
def test_g8_dynca_grads_in_float64(pad):
    g = load("g8_dynca_grads")
    prm = {k: d(g[f"{pad}.{k}"]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
    cond = O.edge_extractor(d(g[f"{pad}.cond_img"]), "tanh")
    x0 = d(g[f"{pad}.x0"]).requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    x = O.dynca_nsteps(x0, cond, [T(u) for u in g[f"{pad}.us"]], p, pad, 0.5)
    ((x * d(g[f"{pad}.cot"])).sum() + (O.dynca_to_rgb(x, 3) * d(g[f"{pad}.cot_rgb"])).sum()).backward()
    assert out_err(x, g[f"{pad}.xT"]) < 1e-5
    assert grad_err(x0.grad, g[f"{pad}.d_x0"]) < 1e-4
    for k in p:
        assert grad_err(p[k].grad, g[f"{pad}.g.{k}"]) < 1e-4, k
    # the helper the GPU tests use returns the same gradients
    _, gx, gw = O.dynca_nsteps_loss_grads(d(g[f"{pad}.x0"]), cond, [T(u) for u in g[f"{pad}.us"]], prm, pad, 0.5,
                                          d(g[f"{pad}.cot"]) + F.pad(2.0 * d(g[f"{pad}.cot_rgb"]), (0, 0, 0, 0, 0, x.shape[1] - 3)))
    assert grad_err(gx, x0.grad) < 1e-12


def test_g10_two_scale_in_float64():
    g = load("g10_two_scale")
    prm = {"w1.weight": d(g["w1"]), "w1.bias": d(g["b1"]), "w2.weight": d(g["w2"]), "w2.bias": d(g["b2"])}
    x, us = d(g["vid.x0"]), T(g["vid.us"])
    cond = O.cpe2d(1, x.shape[2], x.shape[3], dtype=F64)
    assert out_err(O.dynca_perceive_multiscale(x, "circular", (0, 1), cond)[:, :, :12, -12:], g["vid.perc0_crop"]) < 1e-5
    n = 0
    for t in range(us.shape[0]):
        x = O.dynca_step(x, cond, us[t], prm, "circular", 0.5, scales=(0, 1))
        if f"vid.x_t{t + 1}" in g:
            assert out_err(x, g[f"vid.x_t{t + 1}"]) < 1e-5, t
            n += 1
    assert n > 0
    for c in json.loads(str(g["cases"])):
        t_ = c["tag"]
        p = {k: d(g[f"{t_}.{k}"]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
        x0 = d(g[f"{t_}.x0"])
        cnd = (O.edge_extractor(d(g[f"{t_}.cond_img"]), "tanh") if c["cond"] == "edges"
               else O.cpe2d(*[x0.shape[i] for i in (0, 2, 3)], dtype=F64))
        us_ = T(g[f"{t_}.us"])
        assert out_err(O.dynca_step(x0, cnd, us_[0], p, c["pad"], 0.5, scales=(0, 1)), g[f"{t_}.first"]) < 1e-5, c
        assert out_err(O.dynca_nsteps(x0, cnd, list(us_), p, c["pad"], 0.5, scales=(0, 1)), g[f"{t_}.last"]) < 1e-5, c


def test_bf16_faithful_steps_in_float64():
    """cond_step_bf16 / cond_grow_bf16_loss_grads in float64 around the same bf16 roundings: the states agree with the fp32
    form to a bf16 ulp (a final rounding may land on the other side), the gradients to fp32 rounding"""
    g = torch.Generator().manual_seed(5)
    C, hid, B, H, W = 16, 64, 2, 12, 16
    prm = {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
           "update_net.out.0.weight": torch.randn(hid, 3 * C, 1, 1, generator=g) * 0.15,
           "update_net.out.0.bias": torch.randn(hid, generator=g) * 0.1,
           "update_net.out.2.weight": torch.randn(hid, hid, 1, 1, generator=g) * 0.12,
           "update_net.out.2.bias": torch.randn(hid, generator=g) * 0.1,
           "update_net.out.4.weight": torch.randn(C, hid, 1, 1, generator=g) * 0.05}
    prm["update_net.out.4.weight"][3] = 0.0
    x = O._bf(torch.rand(B, C, H, W, generator=g))
    x[:, 3] = O._bf(0.5 + 0.5 * x[:, 3])
    goal = O._bf(torch.randn(B, C, H, W, generator=g) * 0.5)
    us = [torch.rand(B, 1, H, W, generator=g) for _ in range(3)]
    cot = torch.randn(B, C, H, W, generator=g)
    p64 = {k: v.double() for k, v in prm.items()}
    n32 = O.cond_step_bf16(x, goal, us[0], prm)[0]
    n64 = O.cond_step_bf16(x.double(), goal.double(), us[0], p64)[0]
    assert n64.dtype == F64 and torch.equal(O._bf(n64), n64)
    assert float(((n64 - n32.double()).abs() / n32.double().abs().clamp_min(1e-3)).max()) <= 2.0 ** -8
    r32 = O.cond_grow_bf16_loss_grads(x, goal, us, prm, 3, 0.1, 0.5, cot)
    r64 = O.cond_grow_bf16_loss_grads(x.double(), goal.double(), us, p64, 3, 0.1, 0.5, cot.double())
    assert r64[1].dtype == F64
    assert grad_err(r64[1], r32[1]) < 1e-2 and grad_err(r64[2], r32[2]) < 1e-2
    for k in r32[3]:
        assert grad_err(r64[3][k], r32[3][k]) < 1e-2, k
