"""Parity tests proper: the HIP path, called through the C ABI (ctypes), against the CPU oracle
and the golden vectors captured from the reference.  Tolerance: 1e-4 relative fp32 (north_star)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from util import REL_TOL, T, grad_close, grads_match_outside, load, rel_err, sd

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", params=["fast", "generic", "wave"])
def ops(request):
    """Every parity test runs twice: aligned fast-path kernels where the shape allows, and with the
    generic any-shape kernels forced (ncahip_debug_force_generic)."""
    mode = {"fast": 0, "generic": 1, "wave": 2 | 8}[request.param]   # wave: + backward kernel A in the form that is not the mode's default
    with gpu_ops(force=mode) as o:
        o._test_mode = mode
        yield o


def dyn_w(ops, prm, like):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], like)


def cond_w(ops, prm, like):
    return ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                           prm["update_net.out.2.weight"], prm["update_net.out.2.bias"],
                           prm["update_net.out.4.weight"], like)


def rand_dynca_prm(C, fc, c_cond, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    k1 = 4 * C + c_cond
    return {"w1.weight": torch.randn(fc, k1, 1, 1, generator=g) * (0.5 / k1 ** 0.5),
            "w1.bias": torch.randn(fc, generator=g) * 0.1,
            "w2.weight": torch.randn(C, fc, 1, 1, generator=g) * (scale * 0.3 / fc ** 0.5),
            "w2.bias": torch.randn(C, generator=g) * 0.02}


def rand_cond_prm(C, seed, hidden=64, out_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
            "update_net.out.0.weight": torch.randn(hidden, 3 * C, 1, 1, generator=g) * (1.0 / (3 * C) ** 0.5),
            "update_net.out.0.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.2.weight": torch.randn(hidden, hidden, 1, 1, generator=g) * (1.0 / hidden ** 0.5),
            "update_net.out.2.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.4.weight": torch.randn(C, hidden, 1, 1, generator=g) * (out_scale * 0.3 / hidden ** 0.5)}


# ------------------------------------------------------------------ basics
def test_philox_matches_oracle_bit_exact(ops):
    for (B, H, W, seed, step) in ((2, 8, 8, 42, 3), (3, 13, 37, 2 ** 40 + 17, 2 ** 33 + 5), (1, 256, 256, 0, 0)):
        u = ops.philox_uniform(B, H, W, seed, step).cpu().numpy()
        assert np.array_equal(u, O.philox_uniform(seed, step, B, H, W))


@pytest.mark.parametrize("pad", O.PAD_MODES)
@pytest.mark.parametrize("shape", [(2, 12, 12, 16), (1, 16, 64, 64), (3, 5, 13, 37), (1, 3, 2, 2), (2, 4, 1, 8), (1, 2, 9, 1)])
def test_dynca_perceive(ops, pad, shape):
    B, C, H, W = shape
    if pad == "reflect" and (H < 2 or W < 2):
        pytest.skip("F.pad reflect needs >= 2 cells")
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(B * 1000 + W))
    ref = O.dynca_perceive(x, pad)
    got = ops.dynca_perceive(x.to(DEV), pad)
    assert got.shape == ref.shape and rel_err(got, ref) < 1e-5


def test_dynca_perceive_golden_known_answers(ops):
    g = load("g4_perception")
    for pad in O.PAD_MODES:
        for name in ("ramp", "imp"):
            got = ops.dynca_perceive(T(g[name], DEV), pad).cpu().numpy()
            assert np.array_equal(got, g[f"{name}.{pad}"]), (name, pad)  # small integers: exact


@pytest.mark.parametrize("shape", [(2, 12, 32, 32), (1, 16, 16, 64), (2, 5, 7, 9), (1, 3, 1, 1)])
def test_cond_perceive(ops, shape):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(C)
    z, wp = torch.randn(B, C, H, W, generator=gen), torch.randn(3 * C, 1, 3, 3, generator=gen)
    assert rel_err(ops.cond_perceive(z.to(DEV), wp), O.cond_perceive(z, wp)) < 1e-5


# ------------------------------------------------------------------ DyNCA fused step
def test_dynca_step_golden_all_cases(ops):
    g = load("g3_dynca")
    cases = json.loads(str(g["cases"]))
    for c in cases:
        t = c["tag"]
        prm = {k: T(g[f"{t}.{k}"]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
        x0 = T(g[f"{t}.x0"], DEV)
        cond = T(g[f"{t}.cond"], DEV) if f"{t}.cond" in g else None
        w = dyn_w(ops, prm, x0)
        us = T(g[f"{t}.us"], DEV)
        x1 = ops.dynca_step(x0, cond, us[0], w, c["pad"], 0.5)
        assert rel_err(x1, T(g[f"{t}.state_first"])) < REL_TOL, c
        xT, _ = ops.dynca_nsteps(x0, c["T"], cond, us, w, c["pad"], 0.5)
        assert rel_err(xT, T(g[f"{t}.state_last"])) < REL_TOL, c


@pytest.mark.parametrize("C,fc,cc,shape,pad", [
    (12, 96, 3, (2, 40, 72), "circular"), (16, 128, 3, (2, 64, 64), "replicate"), (16, 128, 0, (1, 33, 47), "reflect"),
    (13, 96, 2, (2, 20, 28), "replicate"), (8, 32, 1, (3, 9, 5), "constant"), (16, 100, 4, (1, 8, 32), "circular"),
    (3, 16, 0, (1, 1, 1), "replicate")])
def test_dynca_free_running_64_steps(ops, C, fc, cc, shape, pad):
    """Free-running 64-step parity (no state-dependent threshold in DyNCA, so 1e-4 must hold)."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(C * 100 + W)
    prm = rand_dynca_prm(C, fc, cc, seed=C + fc)
    x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen) * 2 - 1 if cc else None
    Tn = 64
    us = torch.rand(Tn, B, 1, H, W, generator=gen)
    ref = O.dynca_nsteps(x0, cond, list(us), prm, pad, 0.5)
    w = dyn_w(ops, prm, x0.to(DEV))
    got, states = ops.dynca_nsteps(x0.to(DEV), Tn, None if cond is None else cond.to(DEV), us.to(DEV), w, pad, 0.5,
                                   keep_history=True)
    assert float(ref.abs().max()) > 0.3  # the trajectory is non-trivial
    assert rel_err(got, ref) < REL_TOL
    assert states.shape[0] == Tn + 1 and torch.equal(states[Tn], got) and torch.equal(states[0].cpu(), x0)
    got2, _ = ops.dynca_nsteps(x0.to(DEV), Tn, None if cond is None else cond.to(DEV), us.to(DEV), w, pad, 0.5)
    assert torch.equal(got2, got)  # ping-pong ring == history ring, deterministic


def test_dynca_trained_weights_100_steps(ops):
    g = load("g5_real_weights")
    prm = {"w1.weight": T(g["w1"]), "w1.bias": T(g["b1"]), "w2.weight": T(g["w2"]), "w2.bias": T(g["b2"])}
    cond = O.edge_extractor(T(g["cond_img"]), "tanh").to(DEV)
    torch.manual_seed(int(g["rng_seed"]))
    us = torch.stack([torch.rand(1, 1, 48, 48) for _ in range(100)]).to(DEV)
    x = torch.zeros(1, 12, 48, 48, device=DEV)
    w = dyn_w(ops, prm, x)
    _, states = ops.dynca_nsteps(x, 100, cond, us, w, "circular", 0.5, keep_history=True)
    for t in (25, 50, 100):
        assert rel_err(states[t], T(g[f"x_t{t}"])) < REL_TOL, t


def test_dynca_extra_channels_variant(ops):
    g = load("g6_extra_channels")
    prm = {k: T(g[k]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
    x0 = T(g["x0"], DEV)
    w = dyn_w(ops, prm, x0)
    _, states = ops.dynca_nsteps(x0, 5, T(g["pos_emb"], DEV), T(g["us"], DEV), w, "replicate", 0.5, keep_history=True)
    assert rel_err(states[1:], T(g["states"])) < REL_TOL


def test_dynca_inkernel_philox_equals_explicit_u(ops):
    prm = rand_dynca_prm(12, 96, 0, seed=5)
    x0 = (torch.rand(2, 12, 24, 40) - 0.5).to(DEV)
    w = dyn_w(ops, prm, x0)
    a = ops.dynca_step(x0, None, None, w, "circular", 0.5, seed=1234, step=7)
    b = ops.dynca_step(x0, None, ops.philox_uniform(2, 24, 40, 1234, 7), w, "circular", 0.5)
    assert torch.equal(a, b)
    xa, _ = ops.dynca_nsteps(x0, 3, None, None, w, "circular", 0.5, seed=9, step0=100)
    us = torch.stack([ops.philox_uniform(2, 24, 40, 9, 100 + t) for t in range(3)])
    xb, _ = ops.dynca_nsteps(x0, 3, None, us, w, "circular", 0.5)
    assert torch.equal(xa, xb)
    frac = float((a != x0).any(dim=1).float().mean())
    assert 0.4 < frac < 0.6  # ~update_rate of the cells fired


def test_dynca_properties_full_size(ops):
    """BASELINE configs[1] shape (8,16,256,256): size-independent properties + oracle on 2 steps."""
    B, C, H, W, fc = 8, 16, 256, 256, 128
    prm = rand_dynca_prm(C, fc, 3, seed=77)
    gen = torch.Generator().manual_seed(1234)
    x0 = (torch.rand(B, C, H, W, generator=gen) - 0.5)
    cond = torch.rand(B, 3, H, W, generator=gen) * 2 - 1
    us = torch.rand(2, B, 1, H, W, generator=gen)
    xd, cd, ud = x0.to(DEV), cond.to(DEV), us.to(DEV)
    w = dyn_w(ops, prm, xd)
    got, _ = ops.dynca_nsteps(xd, 2, cd, ud, w, "circular", 0.5)
    torch.set_num_threads(max(1, torch.get_num_threads()))
    ref = O.dynca_nsteps(x0, cond, list(us), prm, "circular", 0.5)
    assert rel_err(got, ref) < REL_TOL
    # translation equivariance under circular padding (roll state, cond and u together)
    sh = (5, -9)
    r = lambda t: torch.roll(t, sh, dims=(-2, -1))
    got_r, _ = ops.dynca_nsteps(r(xd).contiguous(), 2, r(cd).contiguous(), r(ud).contiguous(), w, "circular", 0.5)
    assert torch.equal(got_r, r(got))
    # batch independence: sample 3 alone == sample 3 in the batch
    one, _ = ops.dynca_nsteps(xd[3:4], 2, cd[3:4], ud[:, 3:4].contiguous(), w, "circular", 0.5)
    assert torch.equal(one[0], got[3])
    # update_rate 0 => identity; cells whose mask is 0 keep their state exactly
    same = ops.dynca_step(xd, cd, ud[0], w, "circular", 0.0)
    assert torch.equal(same, xd)
    x1 = ops.dynca_step(xd, cd, ud[0], w, "circular", 0.5)
    quiet = (ud[0] + 0.5).floor() == 0
    assert torch.equal(x1[quiet.expand_as(x1)], xd[quiet.expand_as(xd)])


# ------------------------------------------------------------------ ConditionedNCA fused step
def _near_threshold(alpha_pool: torch.Tensor, thr: float, eps: float = 2e-6) -> torch.Tensor:
    return (alpha_pool - thr).abs() < eps


def test_cond_step_golden_g1(ops):
    g = load("g1_cond_step")
    prm = sd(g)
    x, genc, u = T(g["x"], DEV), T(g["genc"], DEV), T(g["u"], DEV)
    a, thr, rate = int(g["alive_ch"]), float(g["thr"]), float(g["fire_rate"])
    w = cond_w(ops, prm, x)
    goal = genc[:, 4:].contiguous()  # unpadded encoder output (8 channels), as the C ABI takes it
    xp, pre = ops.cond_step(x, None, goal, u, w, a, thr, rate)
    assert torch.equal(pre.cpu().bool(), T(g["pre"])[:, 0])
    assert rel_err(xp, T(g["x1"])) < REL_TOL
    x2 = ops.cond_finalize(xp, pre, a, thr)
    # a cell whose pooled new alpha sits within 2e-6 of the threshold may legitimately flip
    pooled = torch.nn.functional.max_pool2d(T(g["x1"])[:, a:a + 1], 3, 1, 1)
    ok = ~_near_threshold(pooled, thr).expand_as(T(g["x2"]))
    assert float(ok.float().mean()) > 0.999
    assert rel_err(x2.cpu()[ok], T(g["x2"])[ok]) < REL_TOL
    assert torch.equal(ops.cond_alive(x, a, thr).cpu(), T(g["pre"]))
    # padded goal (goal_ch == C) is the same computation
    xp2, _ = ops.cond_step(x, None, genc, u, w, a, thr, rate)
    assert torch.equal(xp2, xp)


@pytest.mark.parametrize("tag", ["seed", "rand"])
def test_cond_grow_golden_g2(ops, tag):
    g = load("g2_cond_grow")
    prm = sd(g)
    a = int(g["alive_ch"])
    x0 = T(g[f"{tag}_x0"], DEV)
    goal = T(g["genc"], DEV)
    us = T(g[f"{tag}_us"], DEV)
    ref_states = T(g[f"{tag}_states"])
    w = cond_w(ops, prm, x0)
    Tn = int(g["T"])
    # teacher-forced single steps along the reference trajectory
    prev = x0
    for t in range(Tn):
        xp, pre = ops.cond_step(prev, None, goal, us[t], w, a)
        x2 = ops.cond_finalize(xp, pre, a)
        assert rel_err(x2, ref_states[t]) < REL_TOL, t
        prev = ref_states[t].to(DEV)
    # free-running, pending protocol across steps
    xT, states, pre = ops.cond_grow(x0, Tn, goal, us, w, a, keep_history=True)
    assert rel_err(xT, ref_states[-1]) < REL_TOL
    xT2, _, _ = ops.cond_grow(x0, Tn, goal, us, w, a)
    assert torch.equal(xT2, xT)
    # every intermediate pending state resolves to the reference state
    for t in range(1, Tn + 1):
        assert rel_err(ops.cond_finalize(states[t], pre[t], a), ref_states[t - 1]) < REL_TOL, t


@pytest.mark.parametrize("C,shape,gch,alive", [(12, (2, 32, 32), 8, 3), (16, (2, 48, 80), 12, 3), (16, (1, 21, 35), 16, 3),
                                               (10, (2, 16, 16), 6, 3), (16, (2, 24, 24), 12, -1), (5, (1, 3, 3), 1, 4),
                                               (16, (3, 1, 4), 12, 3), (16, (1, 5, 20), 12, 3), (12, (2, 17, 8), 8, 3),
                                               (16, (1, 4, 36), 0, 3)])
def test_cond_free_running_vs_oracle(ops, C, shape, gch, alive):
    """16 free-running steps vs the oracle.  Alive thresholds make trajectories chaotic near
    alpha==0.1, so cells are compared away from flipped masks; the flip rate itself is bounded."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(C * 7 + W)
    prm = rand_cond_prm(C, seed=C, out_scale=1.0)
    x0 = torch.rand(B, C, H, W, generator=gen)
    if alive >= 0:
        x0[:, alive] = torch.rand(B, H, W, generator=gen) * 0.3
        x0[0, :, : H // 3] = 0.0
    goal = torch.randn(B, gch, H, W, generator=gen)
    Tn = 16
    us = torch.rand(Tn, B, 1, H, W, generator=gen)
    gpad = O.cond_pad_goal(goal, C)
    use_alive = alive >= 0
    ref = x0
    refs = []
    for t in range(Tn):
        ref = O.cond_step(ref, gpad, us[t], prm, max(alive, 0), 0.1, 0.5, use_living_channel=use_alive)
        refs.append(ref)
    w = cond_w(ops, prm, x0.to(DEV))
    got, states, pre = ops.cond_grow(x0.to(DEV), Tn, goal.to(DEV), us.to(DEV), w, alive, keep_history=True)
    bad = ((got.cpu() - ref).abs() > REL_TOL * max(1.0, float(ref.abs().max()))).any(dim=1)
    assert float(bad.float().mean()) < 0.01, float(bad.float().mean())
    # teacher-forced from the oracle's own state at every step: strict
    prev = x0
    for t in range(Tn):
        xp, pr = ops.cond_step(prev.to(DEV), None, goal.to(DEV), us[t].to(DEV), w, alive)
        x2 = ops.cond_finalize(xp, pr, alive).cpu()
        if use_alive:
            x1 = prev + O.cond_fire_mask(us[t], 0.5) * O.cond_update_net(
                O.cond_perceive(prev + gpad * O.cond_alive(prev, alive), prm["perception_net.weight"]), prm)
            near = _near_threshold(torch.nn.functional.max_pool2d(x1[:, alive:alive + 1], 3, 1, 1), 0.1).expand_as(x2)
        else:
            near = torch.zeros_like(x2, dtype=torch.bool)
        assert rel_err(x2[~near], refs[t][~near]) < REL_TOL, t
        prev = refs[t]


def test_cond_dead_grid_stays_dead_and_seed_grows(ops):
    prm = rand_cond_prm(16, seed=3, out_scale=3.0)
    x = torch.zeros(2, 16, 64, 64, device=DEV)
    goal = torch.randn(2, 12, 64, 64, device=DEV)
    w = cond_w(ops, prm, x)
    out, _, _ = ops.cond_grow(x, 8, goal, None, w, 3, seed=1)
    assert float(out.abs().max()) == 0.0  # nothing alive -> pre mask false everywhere -> stays zero
    seed = O.cond_generate_seed(2, 16, 3, 64).to(DEV)
    out, _, _ = ops.cond_grow(seed, 8, goal, None, w, 3, seed=1)
    assert int((out != 0).any(dim=1).sum()) > 2 and float(out.abs().max()) <= 10.0


def test_cond_full_size_cfg2_vs_oracle(ops):
    """BASELINE configs[1]: B=8 C=16 256x256 fp32 forward, 3 steps against the oracle."""
    B, C, H, W = 8, 16, 256, 256
    prm = rand_cond_prm(C, seed=0, out_scale=0.5)
    gen = torch.Generator().manual_seed(1234)
    x0 = torch.rand(B, C, H, W, generator=gen)
    goal = torch.randn(B, 12, H, W, generator=gen) * 0.5
    us = torch.rand(3, B, 1, H, W, generator=gen)
    ref = O.cond_grow(x0, O.cond_pad_goal(goal, C), list(us), prm, 3)
    w = cond_w(ops, prm, x0.to(DEV))
    got, _, _ = ops.cond_grow(x0.to(DEV), 3, goal.to(DEV), us.to(DEV), w, 3)
    bad = ((got.cpu() - ref).abs() > REL_TOL * max(1.0, float(ref.abs().max()))).any(dim=1)
    assert float(bad.float().mean()) < 1e-3
    # in-kernel Philox == explicit uniforms, bit for bit, at full size
    a, _, _ = ops.cond_grow(x0.to(DEV), 2, goal.to(DEV), None, w, 3, seed=5, step0=11)
    ue = torch.stack([ops.philox_uniform(B, H, W, 5, 11 + t) for t in range(2)])
    b, _, _ = ops.cond_grow(x0.to(DEV), 2, goal.to(DEV), ue, w, 3)
    assert torch.equal(a, b)


# ------------------------------------------------------------------ backward (autograd through T steps)
def _grad_close(got, ref, tol=2e-4):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-6)
    return float((got - ref).abs().max()) / scale < tol


def _dynca_gate_ambiguous(x0, cond, us, prm, pad, rate=0.5, k=4e-6):
    """Does the oracle trajectory contain a hidden pre-activation of an UPDATED cell that lies within rounding of zero
    (|w1 y + b1| < k * (|w1| |y| + |b1|), k a few fp32 ulps times the summation-order spread of a 67..131-term dot product)?
    Its ReLU gate may then resolve differently under the MFMA's and the CPU convolution's summation orders, and the gradients that
    pass through that one unit -- dL/dx of its cell and stencil neighbourhood, its row of dW1, its db1 entry -- move by 1e-3 ..
    1e-1 of the maximum (the smaller the model, the more one unit weighs) while the forward and everything else agree to 1e-6.
    Seen once in a few dozen fuzz cases with the scale-3 weights drawn here (seeds 31337 / 90210 / 1)."""
    x = x0
    for u in us:
        r = O.dynca_step(x, cond, u, prm, pad, rate, return_all=True)
        pre = F.conv2d(r["y"], prm["w1.weight"], prm["w1.bias"])
        bound = F.conv2d(r["y"].abs(), prm["w1.weight"].abs(), prm["w1.bias"].abs())
        if bool(((pre.abs() < k * bound) & (r["m"] > 0)).any()):
            return True
        x = r["x"]
    return False


def test_cond_grow_backward_golden_g8(ops):
    """Gradients of <cot, grow(x0)> w.r.t. x0, goal encoding and every weight vs the reference's own autograd."""
    g = load("g8_cond_grads")
    prm = sd(g)
    C, a = g["x0"].shape[1], int(g["alive_ch"])
    x0, gpad, us, cot = T(g["x0"], DEV), T(g["gpad"], DEV), T(g["us"], DEV), T(g["cot"], DEV)
    goal = gpad[:, C - 8:].contiguous()
    w = cond_w(ops, prm, x0)
    Tn = int(g["T"])
    xT, states, pre = ops.cond_grow(x0, Tn, goal, us, w, a, keep_history=True)
    assert rel_err(xT, T(g["xT"])) < REL_TOL
    gr = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, a)
    assert _grad_close(gr["x0"], T(g["d_x0"]))
    assert _grad_close(gr["goal"], T(g["d_gpad"])[:, C - 8:])
    assert _grad_close(gr["wp"].view(3 * C, 1, 3, 3), T(g["grad.perception_net.weight"]))
    assert _grad_close(gr["w1"], T(g["grad.update_net.out.0.weight"])[:, :, 0, 0])
    assert _grad_close(gr["b1"], T(g["grad.update_net.out.0.bias"]))
    assert _grad_close(gr["w2"], T(g["grad.update_net.out.2.weight"])[:, :, 0, 0])
    assert _grad_close(gr["b2"], T(g["grad.update_net.out.2.bias"]))
    assert _grad_close(gr["w3"], T(g["grad.update_net.out.4.weight"])[:, :, 0, 0])
    # deterministic: bitwise identical on a second run
    gr2 = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, a)
    for k in gr:
        assert torch.equal(gr[k], gr2[k]), k


@pytest.mark.parametrize("tag", ["c20", "c32"])
def test_cond_grow_backward_golden_g11_wide(ops, tag):
    """16 < C <= 32 on the fused backward (front + matrix kernels at CP = 20 / 32, stencil adjoint): the reference's DEFAULT
    model (C = 20, nca.py:62-74) and a C = 32 one against the reference's own autograd (G11), 2e-4."""
    g = load("g11_cond_grads_wide")
    prm = {k[len(tag) + 4:]: T(v) for k, v in g.items() if k.startswith(tag + ".sd.")}
    C, a, Tn = g[f"{tag}.x0"].shape[1], int(g[f"{tag}.alive_ch"]), int(g[f"{tag}.T"])
    x0, goal, us, cot = T(g[f"{tag}.x0"], DEV), T(g[f"{tag}.goal_enc"], DEV), T(g[f"{tag}.us"], DEV), T(g[f"{tag}.cot"], DEV)
    w = cond_w(ops, prm, x0)
    xT, states, pre = ops.cond_grow(x0, Tn, goal, us, w, a, keep_history=True)
    assert rel_err(xT, T(g[f"{tag}.xT"])) < REL_TOL
    gr = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, a)
    assert _grad_close(gr["x0"], T(g[f"{tag}.d_x0"]))
    assert _grad_close(gr["goal"], T(g[f"{tag}.d_goal_enc"]))
    assert _grad_close(gr["wp"].view(3 * C, 1, 3, 3), T(g[f"{tag}.grad.perception_net.weight"]))
    assert _grad_close(gr["w1"], T(g[f"{tag}.grad.update_net.out.0.weight"])[:, :, 0, 0])
    assert _grad_close(gr["b1"], T(g[f"{tag}.grad.update_net.out.0.bias"]))
    assert _grad_close(gr["w2"], T(g[f"{tag}.grad.update_net.out.2.weight"])[:, :, 0, 0])
    assert _grad_close(gr["b2"], T(g[f"{tag}.grad.update_net.out.2.bias"]))
    assert _grad_close(gr["w3"], T(g[f"{tag}.grad.update_net.out.4.weight"])[:, :, 0, 0])
    gr2 = ops.cond_grow_backward(states, pre, goal, us, w, cot, Tn, a)   # deterministic: bitwise identical on a second run
    for k in gr:
        assert torch.equal(gr[k], gr2[k]), k


@pytest.mark.parametrize("C,shape,gch,alive,Tn", [(16, (2, 32, 48), 12, 3, 3), (12, (1, 20, 36), 8, 3, 2), (16, (2, 16, 16), 16, -1, 2),
                                                  (20, (2, 32, 48), 16, 3, 3), (24, (1, 20, 36), 20, 3, 2), (32, (2, 24, 16), 28, -1, 2),
                                                  (17, (1, 9, 20), 3, 3, 2), (28, (1, 37, 44), 28, 3, 2), (22, (3, 5, 8), 0, 4, 2)])
def test_cond_grow_backward_vs_oracle_autograd(ops, C, shape, gch, alive, Tn):
    B, H, W = shape
    gen = torch.Generator().manual_seed(C + W)
    prm = rand_cond_prm(C, seed=C + 1, out_scale=2.0)
    x0 = torch.rand(B, C, H, W, generator=gen)
    if alive >= 0:
        x0[0, :, : H // 4] = 0.0
        x0[-1, :, H // 2: H // 2 + 2, 4:8] *= 30.0
    goal = torch.randn(B, gch, H, W, generator=gen) if gch else None
    us = torch.rand(Tn, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    gpad = O.cond_pad_goal(goal, C) if gch else torch.zeros_like(x0)
    xT, dx0, dg, grads = O.cond_grow_loss_grads(x0, gpad, list(us), prm, max(alive, 0), 0.1, 0.5, cot) \
        if alive >= 0 else _oracle_noalive_grads(x0, goal, us, prm, cot, C)
    w = cond_w(ops, prm, x0.to(DEV))
    gd = goal.to(DEV) if gch else None
    _, states, pre = ops.cond_grow(x0.to(DEV), Tn, gd, us.to(DEV), w, alive, keep_history=True)
    gr = ops.cond_grow_backward(states, pre, gd, us.to(DEV), w, cot.to(DEV), Tn, alive)
    assert _grad_close(gr["x0"], dx0)
    if gch:
        assert _grad_close(gr["goal"], dg[:, C - gch:])
    assert _grad_close(gr["wp"].view(3 * C, 1, 3, 3), grads["perception_net.weight"])
    for k, n in (("w1", "update_net.out.0.weight"), ("w2", "update_net.out.2.weight"), ("w3", "update_net.out.4.weight")):
        assert _grad_close(gr[k], grads[n][:, :, 0, 0]), k
    assert _grad_close(gr["b1"], grads["update_net.out.0.bias"]) and _grad_close(gr["b2"], grads["update_net.out.2.bias"])


def _oracle_noalive_grads(x0, goal, us, prm, cot, C, rate=0.5):
    x0 = x0.clone().requires_grad_(True)
    g = (O.cond_pad_goal(goal, C) if goal is not None else torch.zeros_like(x0)).clone().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in prm.items()}
    x = x0
    for u in us:
        x = O.cond_step(x, g, u, p, 0, 0.1, rate, use_living_channel=False)
    (x * cot).sum().backward()
    return x.detach(), x0.grad, g.grad, {k: v.grad for k, v in p.items()}


def test_dynca_nsteps_backward_golden_g8(ops):
    """DyNCA gradients through 4 steps vs the reference's own autograd, all four F.pad modes."""
    g = load("g8_dynca_grads")
    Tn = int(g["T"])
    for pad in O.PAD_MODES:
        prm = {k: T(g[f"{pad}.{k}"]) for k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
        x0 = T(g[f"{pad}.x0"], DEV)
        cond = O.edge_extractor(T(g[f"{pad}.cond_img"]), "tanh").to(DEV)
        us = T(g[f"{pad}.us"], DEV)
        w = dyn_w(ops, prm, x0)
        xT, states = ops.dynca_nsteps(x0, Tn, cond, us, w, pad, 0.5, keep_history=True)
        assert rel_err(xT, T(g[f"{pad}.xT"])) < REL_TOL
        gfin = T(g[f"{pad}.cot"], DEV).clone()
        gfin[:, :3] += 2.0 * T(g[f"{pad}.cot_rgb"], DEV)           # rgb = 2 x[:, :c_out] head (dynca.py:140-141)
        gr = ops.dynca_nsteps_backward(states, cond, us, w, gfin, None, Tn, pad, 0.5)
        assert _grad_close(gr["x0"], T(g[f"{pad}.d_x0"])), pad
        assert _grad_close(gr["w1"], T(g[f"{pad}.g.w1.weight"])[:, :, 0, 0]), pad
        assert _grad_close(gr["b1"], T(g[f"{pad}.g.w1.bias"])), pad
        assert _grad_close(gr["w2"], T(g[f"{pad}.g.w2.weight"])[:, :, 0, 0]), pad
        assert _grad_close(gr["b2"], T(g[f"{pad}.g.w2.bias"])), pad


@pytest.mark.parametrize("C,fc,cc,shape,pad", [(16, 128, 3, (2, 24, 40), "circular"), (12, 96, 0, (1, 9, 13), "reflect"),
                                               (16, 128, 2, (2, 3, 2), "circular"), (8, 32, 1, (1, 1, 5), "replicate")])
def test_dynca_backward_vs_oracle_autograd(ops, C, fc, cc, shape, pad):
    B, H, W = shape
    gen = torch.Generator().manual_seed(C + W)
    prm = rand_dynca_prm(C, fc, cc, seed=3, scale=3.0)
    x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen) if cc else None
    us = torch.rand(3, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    xT, dx0, grads = O.dynca_nsteps_loss_grads(x0, cond, list(us), prm, pad, 0.5, cot)
    w = dyn_w(ops, prm, x0.to(DEV))
    cd = None if cond is None else cond.to(DEV)
    _, states = ops.dynca_nsteps(x0.to(DEV), 3, cd, us.to(DEV), w, pad, 0.5, keep_history=True)
    gr = ops.dynca_nsteps_backward(states, cd, us.to(DEV), w, cot.to(DEV), None, 3, pad, 0.5)
    assert _grad_close(gr["x0"], dx0)
    assert _grad_close(gr["w1"], grads["w1.weight"][:, :, 0, 0]) and _grad_close(gr["b1"], grads["w1.bias"])
    assert _grad_close(gr["w2"], grads["w2.weight"][:, :, 0, 0]) and _grad_close(gr["b2"], grads["w2.bias"])


def test_dynca_c32_forward(ops):
    """BASELINE configs[4] channel count: C = 32 state channels (+3 conditioning) on the forward kernels, fp32 and bf16 storage."""
    from oracle import nca_oracle as O
    C, fc, cc, B, H, W = 32, 128, 3, 1, 24, 40
    g = torch.Generator().manual_seed(32)
    k1 = 4 * C + cc
    prm = {"w1.weight": torch.randn(fc, k1, 1, 1, generator=g) * (0.5 / k1 ** 0.5), "w1.bias": torch.randn(fc, generator=g) * 0.1,
           "w2.weight": torch.randn(C, fc, 1, 1, generator=g) * (0.3 / fc ** 0.5), "w2.bias": torch.randn(C, generator=g) * 0.02}
    x = torch.rand(B, C, H, W, generator=g) - 0.5
    cond = torch.rand(B, cc, H, W, generator=g) * 2 - 1
    us = [torch.rand(B, 1, H, W, generator=g) for _ in range(3)]
    w = ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x.to(DEV))
    for pad in ("circular", "replicate"):
        ref = O.dynca_nsteps(x, cond, us, prm, pad, 0.5)
        got, _ = ops.dynca_nsteps(x.to(DEV), 3, cond.to(DEV), torch.stack(us).to(DEV), w, pad, 0.5)
        assert rel_err(got.cpu(), ref) < REL_TOL
    xb = x.bfloat16()
    gotb, _ = ops.dynca_nsteps(xb.to(DEV), 1, cond.to(DEV), us[0][None].to(DEV), w, "circular", 0.5)
    refb = O.dynca_step(xb.float(), cond, us[0], prm, "circular", 0.5).bfloat16().float()
    assert float(((gotb.float().cpu() - refb).abs() / refb.abs().clamp_min(1.0)).max()) <= 2.0 ** -7


@pytest.mark.parametrize("C,fc,cc", [(32, 256, 3), (16, 192, 0), (12, 320, 2)])
def test_dynca_wide_hidden_forward(ops, C, fc, cc):
    """fc > 128 (SURVEY 8d's cfg5 shape: C = 32, fc = 8C = 256, 3 conditioning channels): one launch per 128-wide slice of
    the hidden layer, the later ones accumulating into x_out -- against the oracle's single sum (dynca.py:117-138), with
    explicit uniforms and with the in-kernel Philox mask (every slice must draw the same mask)."""
    from oracle import nca_oracle as O
    B, H, W = 2, 20, 36
    g = torch.Generator().manual_seed(fc + C)
    k1 = 4 * C + cc
    prm = {"w1.weight": torch.randn(fc, k1, 1, 1, generator=g) * (0.5 / k1 ** 0.5), "w1.bias": torch.randn(fc, generator=g) * 0.1,
           "w2.weight": torch.randn(C, fc, 1, 1, generator=g) * (0.3 / fc ** 0.5), "w2.bias": torch.randn(C, generator=g) * 0.02}
    x = torch.rand(B, C, H, W, generator=g) - 0.5
    cond = torch.rand(B, cc, H, W, generator=g) * 2 - 1 if cc else None
    us = [torch.rand(B, 1, H, W, generator=g) for _ in range(3)]
    w = ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x.to(DEV))
    cd = None if cond is None else cond.to(DEV)
    for pad in ("circular", "reflect"):
        ref = O.dynca_nsteps(x, cond, us, prm, pad, 0.5)
        got, _ = ops.dynca_nsteps(x.to(DEV), 3, cd, torch.stack(us).to(DEV), w, pad, 0.5)
        assert rel_err(got.cpu(), ref) < REL_TOL
    u = ops.philox_uniform(B, H, W, 11, 5, DEV)
    ref1 = O.dynca_step(x, cond, u.cpu(), prm, "replicate", 0.5)
    got1, _ = ops.dynca_nsteps(x.to(DEV), 1, cd, None, w, "replicate", 0.5, seed=11, step0=5)
    assert rel_err(got1.cpu(), ref1) < REL_TOL


def _gram_inputs(ma, nb1, nb2, B, H, W, positive_a=False):
    g = torch.Generator().manual_seed(ma + nb1)
    a = torch.randn(B, ma, H, W, generator=g)
    if positive_a:                                        # non-zero mean: the row sums carry signal
        a = F.relu(a) + 0.1
    b1 = torch.randn(B, nb1, H, W, generator=g)
    b2 = torch.randn(B, nb2, H, W, generator=g) if nb2 else None
    return a.to(DEV), b1.to(DEV), None if b2 is None else b2.to(DEV)


def _gram_rows_check(ops, a, b1, b2, tol_prod=1e-5, tol_rs=1e-5):
    """products and row sums of ops.gram_rows against a float64 contraction (bounds relative to the largest reference entry), the
    fixed summation order, and the accumulate mode: products AND the row-sum tail of the caller's vector"""
    ma, nb = a.shape[1], b1.shape[1] + (0 if b2 is None else b2.shape[1])
    bb = b1 if b2 is None else torch.cat([b1, b2], dim=1)
    ref = torch.einsum("bihw,bjhw->ij", a.double(), bb.double())
    prod, rsum = ops.gram_rows(a, b1, b2)
    scale = float(ref.abs().max())
    assert float((prod.double() - ref).abs().max()) <= tol_prod * scale
    rs_ref = a.double().sum(dim=(0, 2, 3))
    rs_scale = max(1.0, float(rs_ref.abs().max()))
    assert float((rsum.double() - rs_ref).abs().max()) <= tol_rs * rs_scale
    prod2, rsum2 = ops.gram_rows(a, b1, b2)
    assert torch.equal(prod, prod2) and torch.equal(rsum, rsum2)   # fixed summation order
    acc = torch.ones(ma * nb + ma, device=DEV)            # accumulate mode adds to the caller's vector
    ops.gram_rows(a, b1, b2, out=acc)
    assert torch.allclose(acc[:ma * nb].view(ma, -1), prod + 1.0, rtol=0, atol=1e-5 * scale)
    assert torch.allclose(acc[ma * nb:], rsum + 1.0, rtol=0, atol=1e-5 * rs_scale)
    return ref, rs_ref


@pytest.mark.parametrize("ma,nb1,nb2,B,H,W", [(128, 64, 3, 2, 16, 24), (96, 48, 3, 3, 9, 13), (16, 128, 0, 2, 16, 24),
                                               (12, 96, 0, 1, 7, 5), (64, 80, 0, 1, 64, 64), (32, 100, 0, 2, 10, 10),
                                               (5, 3, 0, 1, 1, 1), (40, 64, 3, 1, 1, 1), (1, 1, 0, 2, 3, 5)])
def test_gram_rows(ops, ma, nb1, nb2, B, H, W):
    """ncahip_gram_rows_f32 (the DyNCA weight-gradient products, cell axis as K) against a float64 contraction: row counts
    that do not fill the 16-row tiles, cell counts that do not fill the 64-cell chunks, the two-tensor B operand; a single cell
    (HW = 1, B = 1) and a single row against a single row (ma = nb = 1)."""
    _gram_rows_check(ops, *_gram_inputs(ma, nb1, nb2, B, H, W))


# (ma, nb1, nb2): <2,9>, <1,9>, the small-ma fall-through to <1,9> (ma <= 32 but nb > 128), and nb = 144 = 16 NB_T, where the ones
# column does not fit and the vector-add form must be taken even when NCAHIP_GRAM_ONES=1 asks for it
GRAM_WIDE = [(128, 128, 3), (40, 80, 4), (8, 128, 4), (128, 141, 3)]


@pytest.mark.parametrize("ma,nb1,nb2,B,H,W,ones", [(*s, 3, 9, 13, o) for s in GRAM_WIDE for o in (None, "0", "1")] +
                         [(128, 64, 3, 2, 16, 24, "1")])       # nb = 67 (<2,5>): the ones column is not its default
def test_gram_rows_row_sum_forms(ops, monkeypatch, ma, nb1, nb2, B, H, W, ones):
    """gram_rows_kernel<*,9,true> and both forms of the row sums (vector adds beside the MFMAs / one more B column of ones): the
    launcher reads NCAHIP_GRAM_ONES per launch (tools/ab_gram.py relies on that), unset = the template's default"""
    if ones is None:
        monkeypatch.delenv("NCAHIP_GRAM_ONES", raising=False)
    else:
        monkeypatch.setenv("NCAHIP_GRAM_ONES", ones)
    _gram_rows_check(ops, *_gram_inputs(ma, nb1, nb2, B, H, W, positive_a=True))


def test_gram_rows_grid_stride(ops):
    """more chunks than workgroups: the grid-stride loop with the next chunk prefetched.  The grid is min(chunks, 2 CUs); ten
    workgroups take a second chunk, HW is no multiple of 64.  A dropped or doubled chunk moves a row sum by 1 / 500.  K = B HW is
    about 3e4 here, so the bound is ten times the error of the plain fp32 torch contraction of the same inputs against float64, or
    1e-5, whichever is larger (the convention of tests/test_gpu_slw.py and tests/test_gpu_ot_moment.py)."""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    B, ma, nb, HW = 2, 16, 20, 64 * (cus + 4) + 37
    assert B * ((HW + 63) // 64) > 2 * cus and HW % 64 != 0
    a, b1, _ = _gram_inputs(ma, nb, 0, B, 1, HW, positive_a=True)
    ref = torch.einsum("bihw,bjhw->ij", a.double(), b1.double())
    rs_ref = a.double().sum(dim=(0, 2, 3))
    e_prod = float((torch.einsum("bihw,bjhw->ij", a, b1).double() - ref).abs().max()) / float(ref.abs().max())
    e_rs = float((a.sum(dim=(0, 2, 3)).double() - rs_ref).abs().max()) / float(rs_ref.abs().max())
    tol_prod, tol_rs = max(10 * e_prod, 1e-5), max(10 * e_rs, 1e-5)
    prod, rsum = ops.gram_rows(a, b1)
    g_prod = float((prod.double() - ref).abs().max()) / float(ref.abs().max())
    g_rs = float((rsum.double() - rs_ref).abs().max()) / float(rs_ref.abs().max())
    print(f"\ngram_rows grid stride, {B * ((HW + 63) // 64)} chunks on {2 * cus} workgroups: products {g_prod:.2e} (fp32 torch "
          f"{e_prod:.2e}, bound {tol_prod:.2e}), row sums {g_rs:.2e} (fp32 torch {e_rs:.2e}, bound {tol_rs:.2e})")
    _gram_rows_check(ops, a, b1, None, tol_prod, tol_rs)


@pytest.mark.parametrize("C,fc,cc,H,W", [(16, 128, 3, 24, 40), (12, 96, 0, 13, 36), (8, 64, 2, 9, 20)])
def test_dynca_bwd_fused_w2_matches_buffers(ops, C, fc, cc, H, W):
    """The two backward entry points agree: ncahip_dynca_step_bwd_w2_f32 (layer-2 gradient accumulated inside the step kernel,
    h never written) against ncahip_dynca_step_bwd_f32 + ncahip_gram_rows_f32 on its h / dh buffers, and both against a
    float64 contraction of those buffers."""
    from ncahip import _capi
    B = 2
    g_ = torch.Generator().manual_seed(C * fc)
    prm = rand_dynca_prm(C, fc, cc, seed=5, scale=3.0)
    x = (torch.rand(B, C, H, W, generator=g_) - 0.5).to(DEV)
    cond = torch.rand(B, cc, H, W, generator=g_).to(DEV) if cc else None
    u = torch.rand(B, 1, H, W, generator=g_).to(DEV)
    gn = torch.randn(B, C, H, W, generator=g_).to(DEV)
    w = dyn_w(ops, prm, x)
    L, P = ops.lib(), ops._p
    hb, dh, dy = (torch.empty(B, fc, H, W, device=DEV), torch.empty(B, fc, H, W, device=DEV), torch.empty(B, 4 * C, H, W, device=DEV))
    gx = torch.empty_like(gn)
    _capi.check(L.ncahip_dynca_step_bwd_f32(P(x), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, 2, 0.5,
                                            0, 0, P(gn), P(gx), P(hb), P(dh), P(dy), None), "bwd")
    do = gn * (u + 0.5).floor()
    w2_a, b2_a = ops.gram_rows(do, hb)
    dh2, dy2, gx2 = torch.empty_like(dh), torch.empty_like(dy), torch.empty_like(gn)
    out = torch.empty(C * fc + C, device=DEV)
    nws = L.ncahip_dynca_step_bwd_w2_workspace(B, C, H, W, fc)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    _capi.check(L.ncahip_dynca_step_bwd_w2_f32(P(x), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, 2, 0.5,
                                               0, 0, P(gn), P(gx2), P(dh2), P(dy2), P(out), 0, P(ws), nws, None), "bwd_w2")
    assert torch.equal(gx, gx2) and torch.equal(dh, dh2)
    ref = torch.einsum("bihw,bjhw->ij", do.double().cpu(), hb.double().cpu())
    scale = max(1e-6, float(ref.abs().max()))
    assert float((out[:C * fc].view(C, fc).cpu().double() - ref).abs().max()) <= 2e-5 * scale
    assert float((w2_a.cpu().double() - ref).abs().max()) <= 2e-5 * scale
    rs = do.double().sum(dim=(0, 2, 3)).cpu()
    assert float((out[C * fc:].cpu().double() - rs).abs().max()) <= 2e-5 * max(1.0, float(rs.abs().max()))


@pytest.mark.parametrize("cset", [(5, 8, 12, 13, 16), (17, 18, 20, 20, 24)], ids=["narrow", "wide"])
def test_cond_step_shape_fuzz(ops, cset):
    """Seeded random shapes / channel counts / goal widths / alive settings / fire rates, pending inputs included: one
    teacher-forced step each against the oracle (nca.py:181-195).  Covers tiles that straddle every image edge and the
    aligned / unaligned dispatch boundary (W % 4).  `wide`: 16 < C <= 20 runs the producer/consumer kernel's wide LDS carve
    (tile buffers on top of the dead weight images), C = 24 the generic kernel."""
    rng = np.random.RandomState(int(os.environ.get("NCAHIP_FUZZ_SEED", "1234")) + (0 if cset[0] == 5 else 77))   # wider sweeps: NCAHIP_FUZZ_SEED / _CASES
    for case in range(int(os.environ.get("NCAHIP_FUZZ_CASES", "24"))):
        C = int(rng.choice(cset))
        B = int(rng.randint(1, 4)); H = int(rng.randint(1, 41)); W = int(rng.randint(1, 53))
        if rng.rand() < 0.6:
            W = max(4, (W // 4) * 4)                               # exercise the aligned kernels more often
        alive = int(rng.choice([-1, 3, min(4, C - 1)]))
        gch = int(rng.choice([0, 1, max(1, C - 4), C]))
        rate = float(rng.choice([0.0, 0.5, 1.0]))
        gen = torch.Generator().manual_seed(1000 + case)
        prm = rand_cond_prm(C, seed=case, out_scale=2.0)
        x = torch.rand(B, C, H, W, generator=gen) * 1.4 - 0.2
        if alive >= 0:
            x[:, alive] = torch.rand(B, H, W, generator=gen) * 0.4
        goal = torch.randn(B, gch, H, W, generator=gen) if gch else None
        u = torch.rand(B, 1, H, W, generator=gen)
        gpad = O.cond_pad_goal(goal, C) if goal is not None else torch.zeros_like(x)
        d = O.cond_step(x, gpad, u, prm, max(alive, 0), 0.1, rate, use_living_channel=alive >= 0, return_all=True)
        w = cond_w(ops, prm, x.to(DEV))
        xp, pre = ops.cond_step(x.to(DEV), None, None if goal is None else goal.to(DEV), u.to(DEV), w, alive, 0.1, rate)
        tag = (case, C, B, H, W, alive, gch, rate)
        assert rel_err(xp.cpu(), d["x1"]) < REL_TOL, tag
        if alive >= 0:
            assert torch.equal(pre.cpu().bool(), d["pre"][:, 0]), tag
        # second step from the pending state == oracle step from the resolved state (pending protocol)
        u2 = torch.rand(B, 1, H, W, generator=gen)
        x2ref = d["x2"]
        ac = max(alive, 0)
        near = (_near_threshold(torch.nn.functional.max_pool2d(d["x1"][:, ac:ac + 1], 3, 1, 1), 0.1)
                if alive >= 0 else torch.zeros(B, 1, H, W, dtype=torch.bool))
        if bool(near.any()):
            continue                                               # a cell on the life threshold: trajectories may split
        d2 = O.cond_step(x2ref, gpad, u2, prm, max(alive, 0), 0.1, rate, use_living_channel=alive >= 0, return_all=True)
        xp2, _ = ops.cond_step(xp, pre, None if goal is None else goal.to(DEV), u2.to(DEV), w, alive, 0.1, rate)
        assert rel_err(xp2.cpu(), d2["x1"]) < REL_TOL, tag


def test_many_small_items_and_side_stream(ops):
    """B = 67 grids of 20 x 20 (more super-tiles than workgroup slots per XCD chunk, ragged tile edges, batch offsets) for the
    forward and backward of both models against the oracle, launched on a non-default stream."""
    B, H, W = 67, 20, 20
    gen = torch.Generator().manual_seed(67)
    side = torch.cuda.Stream()
    # ConditionedNCA, C = 16, two steps
    C = 16
    prm = rand_cond_prm(C, seed=4, out_scale=2.0)
    x0 = torch.rand(B, C, H, W, generator=gen) * 1.4 - 0.2
    x0[:, 3] = torch.rand(B, H, W, generator=gen) * 0.4
    goal = torch.randn(B, 12, H, W, generator=gen)
    us = torch.rand(2, B, 1, H, W, generator=gen)
    cot = torch.randn(B, C, H, W, generator=gen)
    gpad = O.cond_pad_goal(goal, C)
    ref = O.cond_grow(x0, gpad, list(us), prm, 3)
    w = cond_w(ops, prm, x0.to(DEV))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out, states, pre = ops.cond_grow(x0.to(DEV), 2, goal.to(DEV), us.to(DEV), w, 3, keep_history=True)
        gr = ops.cond_grow_backward(states, pre, goal.to(DEV), us.to(DEV), w, cot.to(DEV), 2, 3)
    side.synchronize()
    assert rel_err(out.cpu(), ref) < REL_TOL
    d1 = O.cond_step(x0, gpad, us[0], prm, 3, 0.1, 0.5, use_living_channel=True, return_all=True)
    pools = [torch.nn.functional.max_pool2d(t[:, 3:4], 3, 1, 1) for t in (x0, d1["x1"], d1["x2"], ref)]
    if not any(bool(_near_threshold(pl, 0.1, 1e-5).any()) for pl in pools):
        _, dx0, dg, grads = O.cond_grow_loss_grads(x0, gpad, list(us), prm, 3, 0.1, 0.5, cot)
        assert _grad_close(gr["x0"], dx0) and _grad_close(gr["goal"], dg[:, C - 12:])
        assert _grad_close(gr["w1"], grads["update_net.out.0.weight"][:, :, 0, 0])
        assert _grad_close(gr["wp"].view(3 * C, 1, 3, 3), grads["perception_net.weight"])
    # DyNCA, C = 12, fc = 96, reflect padding, two steps
    C, fc, cc = 12, 96, 3
    dp = rand_dynca_prm(C, fc, cc, seed=6, scale=3.0)
    xd = torch.rand(B, C, H, W, generator=gen) - 0.5
    cond = torch.rand(B, cc, H, W, generator=gen)
    ud = torch.rand(2, B, 1, H, W, generator=gen)
    cd_ = torch.randn(B, C, H, W, generator=gen)
    xT, dx0, grads = O.dynca_nsteps_loss_grads(xd, cond, list(ud), dp, "reflect", 0.5, cd_)
    dwt = dyn_w(ops, dp, xd.to(DEV))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outd, st = ops.dynca_nsteps(xd.to(DEV), 2, cond.to(DEV), ud.to(DEV), dwt, "reflect", 0.5, keep_history=True)
        gd = ops.dynca_nsteps_backward(st, cond.to(DEV), ud.to(DEV), dwt, cd_.to(DEV), None, 2, "reflect", 0.5)
    side.synchronize()
    assert rel_err(outd.cpu(), xT) < REL_TOL
    assert _grad_close(gd["x0"], dx0) and _grad_close(gd["w1"], grads["w1.weight"][:, :, 0, 0]) and _grad_close(gd["w2"], grads["w2.weight"][:, :, 0, 0])
    assert _grad_close(gd["b1"], grads["w1.bias"]) and _grad_close(gd["b2"], grads["w2.bias"])


def test_cond_large_plane_tile_vs_generic(ops):
    """Planes of 2^22 cells and more (plane bytes >= 2^24): the tile kernels' in-plane byte offsets must not go through 24-bit
    multiplies.  The CPU oracle is out of reach at this size; the any-shape kernels (oracle-checked at every small shape)
    are the reference here.  1 x 12 x 1024 x 4096, two steps, in-kernel Philox mask."""
    if ops._test_mode != 0:
        pytest.skip("compares the two kernel families itself; run once")
    B, C, H, W = 1, 12, 1024, 4096
    gen = torch.Generator().manual_seed(9)
    prm = rand_cond_prm(C, seed=9, out_scale=2.0)
    x = torch.rand(B, C, H, W, generator=gen).to(DEV)
    goal = (torch.randn(B, 8, H, W, generator=gen) * 0.5).to(DEV)
    w = cond_w(ops, prm, x)
    outs = []
    try:
        for force in (0, 1):
            ops.force_generic(force)
            o, _, _ = ops.cond_grow(x, 2, goal, None, w, 3, seed=7)
            outs.append(o)
    finally:
        ops.force_generic(ops._test_mode)
    assert float((outs[0] - outs[1]).abs().max()) <= 1e-6 * max(1.0, float(outs[1].abs().max()))


@pytest.mark.parametrize("C,hidden", [(20, 64), (18, 48)])
def test_cond_default_model_tile_vs_generic(ops, C, hidden):
    """The reference's default channel count C = 20 (nca.py:62-94) at the bench size 8 x C x 256^2, 6 free-running steps with the
    in-kernel mask: every workgroup of the producer/consumer kernel walks several rounds, so the second tile buffers -- which
    live on top of the W1 / W2 images once the consumers hold those in registers -- are reused many times.  Reference: the
    any-shape kernel family (oracle-checked at every small shape; the CPU oracle needs minutes at this size)."""
    if ops._test_mode != 0:
        pytest.skip("compares the two kernel families itself; run once")
    B, H, W = 8, 256, 256
    gen = torch.Generator().manual_seed(20)
    prm = rand_cond_prm(C, seed=20, hidden=hidden, out_scale=2.0)
    x = torch.rand(B, C, H, W, generator=gen).to(DEV)
    goal = (torch.randn(B, C - 4, H, W, generator=gen) * 0.5).to(DEV)
    w = cond_w(ops, prm, x)
    outs = []
    try:
        for force in (0, 1):
            ops.force_generic(force)
            o, _, _ = ops.cond_grow(x, 6, goal, None, w, 3, seed=11)
            outs.append(o)
    finally:
        ops.force_generic(ops._test_mode)
    assert float((outs[0] - outs[1]).abs().max()) <= 2e-6 * max(1.0, float(outs[1].abs().max()))
    assert float(outs[0].abs().max()) > 0.5 and bool(torch.isfinite(outs[0]).all())


def test_cond_backward_shape_fuzz(ops):
    """Seeded random shapes / channel counts (C below the kernels' padded widths included) / goal widths / alive settings for
    ONE backward step against the oracle's autograd (conditioned_trainer.py:125-132).  Cases with a cell on the life
    threshold are skipped (the mask's derivative is zero almost everywhere; on the threshold the two sides disagree)."""
    rng = np.random.RandomState(int(os.environ.get("NCAHIP_FUZZ_SEED", "777")))
    done = 0
    for case in range(int(os.environ.get("NCAHIP_FUZZ_CASES", "16"))):
        C = int(rng.choice([5, 8, 12, 13, 16, 17, 20, 23, 24, 29, 32]))
        B = int(rng.randint(1, 3)); H = int(rng.randint(1, 25)); W = 4 * int(rng.randint(1, 11))
        alive = int(rng.choice([-1, 3, min(4, C - 1)]))
        gch = int(rng.choice([0, 1, max(1, C - 4), C]))
        rate = float(rng.choice([0.5, 0.5, 0.0, 1.0]))
        philox = bool(rng.rand() < 0.4)            # in-kernel mask: the oracle gets the same uniforms from ncahip_philox_uniform
        gen = torch.Generator().manual_seed(3000 + case)
        prm = rand_cond_prm(C, seed=case, out_scale=2.0)
        x0 = torch.rand(B, C, H, W, generator=gen) * 1.4 - 0.2
        if alive >= 0:
            x0[:, alive] = torch.rand(B, H, W, generator=gen) * 0.4
        goal = torch.randn(B, gch, H, W, generator=gen) if gch else None
        us = torch.rand(1, B, 1, H, W, generator=gen)
        if philox:
            us = ops.philox_uniform(B, H, W, 17 + case, 5, DEV).cpu()[None]
        cot = torch.randn(B, C, H, W, generator=gen)
        gpad = O.cond_pad_goal(goal, C) if gch else torch.zeros_like(x0)
        if alive >= 0:
            d = O.cond_step(x0, gpad, us[0], prm, alive, 0.1, rate, use_living_channel=True, return_all=True)
            pools = [torch.nn.functional.max_pool2d(t[:, alive:alive + 1], 3, 1, 1) for t in (x0, d["x1"])]
            if any(bool(_near_threshold(pl, 0.1, 1e-5).any()) for pl in pools):
                continue
            xT, dx0, dg, grads = O.cond_grow_loss_grads(x0, gpad, list(us), prm, alive, 0.1, rate, cot)
        else:
            xT, dx0, dg, grads = _oracle_noalive_grads(x0, gpad[:, C - gch:] if gch else None, us, prm, cot, C, rate)
        w = cond_w(ops, prm, x0.to(DEV))
        gd, ud = (None if goal is None else goal.to(DEV)), (None if philox else us.to(DEV))
        _, states, pre = ops.cond_grow(x0.to(DEV), 1, gd, ud, w, alive, fire_rate=rate, seed=17 + case, step0=5, keep_history=True)
        gr = ops.cond_grow_backward(states, pre, gd, ud, w, cot.to(DEV), 1, alive, fire_rate=rate, seed=17 + case, step0=5)
        tag = (case, C, B, H, W, alive, gch, rate, philox)
        assert _grad_close(gr["x0"], dx0), tag
        if gch:
            assert _grad_close(gr["goal"], dg[:, C - gch:]), tag
        assert _grad_close(gr["wp"].view(3 * C, 1, 3, 3), grads["perception_net.weight"]), tag
        for k, n in (("w1", "update_net.out.0.weight"), ("w2", "update_net.out.2.weight"), ("w3", "update_net.out.4.weight")):
            assert _grad_close(gr[k], grads[n][:, :, 0, 0]), (k,) + tag
        assert _grad_close(gr["b1"], grads["update_net.out.0.bias"]) and _grad_close(gr["b2"], grads["update_net.out.2.bias"]), tag
        done += 1
    assert done > 0


def test_dynca_backward_shape_fuzz(ops):
    """Seeded random shapes / pad modes / conditioning widths / layer widths for the DyNCA backward (two steps) against the
    oracle's autograd: the fused layer-2 product, the cell-axis-as-K layer-1 product, the vectorised and the border-band
    stencil adjoint all see odd sizes here."""
    rng = np.random.RandomState(int(os.environ.get("NCAHIP_FUZZ_SEED", "888")))
    pads = ["replicate", "circular", "reflect", "constant"]
    ncases, ambiguous = int(os.environ.get("NCAHIP_FUZZ_CASES", "14")), 0
    shapes = [(12, 96), (16, 128), (8, 64), (16, 96), (5, 40), (32, 256), (20, 100), (24, 192), (16, 320), (32, 128)]
    for case in range(ncases):
        # (round 2: C up to 32 and hidden layers beyond 128 -- 128-wide slices -- through the C driver as well; the multi-slice
        # shapes (32, 256), (16, 320), (24, 192) are always in the draw: cases 0..2)
        C, fc = shapes[int(rng.randint(0, 10))]
        if case < 3:
            C, fc = ((32, 256), (16, 320), (24, 192))[case]
        cc = int(rng.choice([0, 2, 3]))
        B = int(rng.randint(1, 3)); H = int(rng.randint(2, 30)); W = int(rng.randint(2, 45))
        if rng.rand() < 0.5:
            W = max(4, (W // 4) * 4)
        pad = pads[int(rng.randint(0, 4))]
        gen = torch.Generator().manual_seed(4000 + case)
        prm = rand_dynca_prm(C, fc, cc, seed=case, scale=3.0)
        x0 = torch.rand(B, C, H, W, generator=gen) - 0.5
        cond = torch.rand(B, cc, H, W, generator=gen) if cc else None
        us = torch.rand(2, B, 1, H, W, generator=gen)
        cot = torch.randn(B, C, H, W, generator=gen)
        xT, dx0, grads = O.dynca_nsteps_loss_grads(x0, cond, list(us), prm, pad, 0.5, cot)
        w = dyn_w(ops, prm, x0.to(DEV))
        cd = None if cond is None else cond.to(DEV)
        _, states = ops.dynca_nsteps(x0.to(DEV), 2, cd, us.to(DEV), w, pad, 0.5, keep_history=True)
        gr = ops.dynca_nsteps_backward(states, cd, us.to(DEV), w, cot.to(DEV), None, 2, pad, 0.5)
        tag = (case, C, fc, cc, B, H, W, pad)
        ok = (_grad_close(gr["x0"], dx0) and _grad_close(gr["w1"], grads["w1.weight"][:, :, 0, 0]) and _grad_close(gr["b1"], grads["w1.bias"])
              and _grad_close(gr["w2"], grads["w2.weight"][:, :, 0, 0]) and _grad_close(gr["b2"], grads["w2.bias"]))
        if not ok:
            # Not skipped: a case that misses the max-norm bound must (i) agree in the forward, (ii) have a hidden
            # pre-activation of an updated cell within rounding of zero in the ORACLE's own trajectory (the gate may then
            # legitimately resolve differently: see the helper), (iii) agree at 2e-4 in dL/dx0 everywhere OUTSIDE the influence
            # region of those gates (a wrong slice offset or tile mapping shows up there), and (iv) keep every weight gradient
            # within 5 % relative L2 (in these small problems one hidden unit of one cell weighs up to ~1e-1 of a gradient entry)
            assert rel_err(states[-1].cpu(), xT) < 1e-5 and _dynca_gate_ambiguous(x0, cond, list(us), prm, pad), tag
            region, count = O.dynca_gate_influence(x0, cond, list(us), prm, pad, 4e-6)
            ok_out, n_out, n_in = grads_match_outside(gr["x0"], dx0, region)
            assert int(count.sum()) > 0 and ok_out, tag + (n_out, n_in)
            for got, ref in ((gr["w1"], grads["w1.weight"][:, :, 0, 0]), (gr["b1"], grads["w1.bias"]),
                             (gr["w2"], grads["w2.weight"][:, :, 0, 0]), (gr["b2"], grads["w2.bias"])):
                assert grad_close(got, ref, l2=5e-2, cap=2e-1), tag
            ambiguous += 1
    assert 7 * ambiguous <= ncases, (ambiguous, ncases)      # five seeds x 64 cases in round 2 showed at most 1 in 16


def test_dynca_step_shape_fuzz(ops):
    """Seeded random shapes / pad modes / conditioning widths for the DyNCA step (dynca.py:117-138)."""
    rng = np.random.RandomState(int(os.environ.get("NCAHIP_FUZZ_SEED", "4321")))
    pads = ["replicate", "circular", "reflect", "constant"]
    for case in range(int(os.environ.get("NCAHIP_FUZZ_CASES", "16"))):
        C, fc = [(12, 96), (16, 128), (8, 64), (16, 96), (32, 128)][int(rng.randint(0, 5))]
        cc = int(rng.choice([0, 2, 3]))
        B = int(rng.randint(1, 3)); H = int(rng.randint(2, 37)); W = int(rng.randint(2, 45))
        pad = pads[int(rng.randint(0, 4))]
        gen = torch.Generator().manual_seed(2000 + case)
        k1 = 4 * C + cc
        prm = {"w1.weight": torch.randn(fc, k1, 1, 1, generator=gen) * (0.5 / k1 ** 0.5), "w1.bias": torch.randn(fc, generator=gen) * 0.1,
               "w2.weight": torch.randn(C, fc, 1, 1, generator=gen) * (0.3 / fc ** 0.5), "w2.bias": torch.randn(C, generator=gen) * 0.02}
        x = torch.rand(B, C, H, W, generator=gen) - 0.5
        cond = (torch.rand(B, cc, H, W, generator=gen) * 2 - 1) if cc else None
        u = torch.rand(B, 1, H, W, generator=gen)
        rate = float(rng.choice([0.25, 0.5, 1.0]))
        ref = O.dynca_step(x, cond, u, prm, pad, rate)
        w = ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x.to(DEV))
        got, _ = ops.dynca_nsteps(x.to(DEV), 1, None if cond is None else cond.to(DEV), u[None].to(DEV), w, pad, rate)
        assert rel_err(got.cpu(), ref) < REL_TOL, (case, C, fc, cc, B, H, W, pad, rate)


def test_device_error_word_plumbing(ops):
    """A hand-off poll that expires sets a sticky host-visible error word; the grow drivers then refuse with NCAHIP_EDEVICE and
    ncahip_check_errors reports and clears it.  (The expiry itself cannot be provoked on a healthy device: the test hook sets
    the word exactly as the kernel does.)"""
    from ncahip._capi import NcaHipError
    prm = rand_cond_prm(16, seed=1)
    x = torch.rand(1, 16, 32, 32, device=DEV)
    w = cond_w(ops, prm, x)
    ops.cond_grow(x, 2, None, None, w, 3)
    ops.check_errors()                                   # clean device: no error
    assert ops.lib().ncahip_debug_inject_error(1) == 0
    with pytest.raises(NcaHipError, match="hand-off"):
        ops.cond_grow(x, 2, None, None, w, 3)            # refused before anything is enqueued
    with pytest.raises(NcaHipError, match="error word"):
        ops.check_errors()                               # reported once, and cleared
    ops.check_errors()
    out, _, _ = ops.cond_grow(x, 2, None, None, w, 3)
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ fire masks as bits (include/ncahip.h: NCAHIP_SEED_U_IS_BITS)
def test_pack_fire_mask_matches_the_step_predicates(ops):
    """ncahip_pack_fire_mask_u32 evaluates exactly nca.py:171-174 / dynca.py:131 (odd cell counts: partial last word, rates at
    and beyond the interval ends) and unpack_fire_mask inverts it."""
    gen = torch.Generator().manual_seed(5)
    for (Tn, B, H, W) in ((3, 2, 7, 9), (1, 1, 1, 1), (2, 3, 16, 32), (1, 1, 5, 13)):
        u = torch.rand(Tn, B, 1, H, W, generator=gen)
        u[0, 0, 0, 0, 0] = 0.0
        u.view(-1)[-1] = 0.99999994
        for mode, rates in (("cond", (0.5, 0.0, 1.0, 0.25, 1.5, -0.5)), ("dynca", (0.5, 0.0, 0.25, 0.9))):
            for rate in rates:
                ref = (u.clamp(0, 1) < rate).float() if mode == "cond" else (u + rate).floor()
                bits = ops.pack_fire_mask(u.to(DEV), rate, mode)
                assert bits.shape == (Tn, (B * H * W + 31) // 32)
                assert torch.equal(ops.unpack_fire_mask(bits, B, H, W).cpu(), ref), (mode, rate, Tn, B, H, W)
                pad_bits = B * H * W % 32          # bits past the last cell are zero
                if pad_bits:
                    assert int((bits[:, -1].cpu().to(torch.int64) & 0xFFFFFFFF).max()) < (1 << pad_bits)


def test_draw_fire_masks_follows_the_rand_like_stream(ops):
    """The drop-in classes' mask source: per step ONE [B,1,H,W] float32 draw from the device's global generator, exactly the
    reference's call (nca.py:172), evaluated to bits.  Same values and same generator position as T rand_like calls."""
    x = torch.zeros(3, 16, 20, 28, device=DEV)
    for steps in (1, 5, 37):
        torch.manual_seed(1234)
        ref = torch.stack([torch.rand_like(x[:, 0:1]) for _ in range(steps)])
        st_ref = torch.cuda.get_rng_state()
        torch.manual_seed(1234)
        bits = ops.draw_fire_masks(3, 20, 28, steps, 0.5, "cond", x.device)
        assert torch.equal(torch.cuda.get_rng_state(), st_ref)
        assert torch.equal(ops.unpack_fire_mask(bits, 3, 20, 28), (ref.clamp(0, 1) < 0.5).float())
        torch.manual_seed(1234)
        ref2 = torch.stack([torch.rand(3, 1, 20, 28, device=DEV) for _ in range(steps)])      # dynca.py:131's call
        assert torch.equal(ref2, ref)


@pytest.mark.parametrize("C,shape,dt", [(16, (2, 32, 48), torch.float32), (12, (1, 19, 36), torch.float32), (16, (2, 16, 64), torch.bfloat16),
                                        (20, (1, 24, 40), torch.float32)])
def test_cond_grow_with_bit_masks_equals_float_uniforms(ops, C, shape, dt):
    """Forward and backward of the grow loop: bit-packed masks in place of the float draws give bit-identical results, every
    kernel family (tile kernels, generic kernels, the backward's front kernel)."""
    B, H, W = shape
    if dt == torch.bfloat16 and getattr(ops, "_test_mode", 0) & 1:
        pytest.skip("bf16 storage: tile kernels only")
    gen = torch.Generator().manual_seed(C + W)
    prm = rand_cond_prm(C, seed=C, out_scale=1.5)
    x0 = torch.rand(B, C, H, W, generator=gen).to(DEV, dt)
    goal = torch.randn(B, C - 4, H, W, generator=gen).to(DEV, dt)
    Tn = 3
    us = torch.rand(Tn, B, 1, H, W, generator=gen).to(DEV)
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    w = cond_w(ops, prm, x0)
    for rate in (0.5, 0.2):
        bits = ops.pack_fire_mask(us, rate, "cond")
        o1, s1, p1 = ops.cond_grow(x0, Tn, goal, us, w, 3, fire_rate=rate, keep_history=True)
        o2, s2, p2 = ops.cond_grow(x0, Tn, goal, bits, w, 3, fire_rate=rate, keep_history=True)
        assert torch.equal(o1, o2) and torch.equal(s1, s2) and torch.equal(p1[1:], p2[1:])      # (pre[0] is never written: the input is a true state)
        if W % 4 == 0:
            g1 = ops.cond_grow_backward(s1, p1, goal, us, w, cot, Tn, 3, fire_rate=rate)
            g2 = ops.cond_grow_backward(s2, p2, goal, bits, w, cot, Tn, 3, fire_rate=rate)
            for k in g1:
                assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("C,fc,shape,two", [(12, 96, (2, 20, 28), False), (16, 128, (1, 16, 32), True), (32, 256, (1, 9, 13), False)])
def test_dynca_nsteps_with_bit_masks_equals_float_uniforms(ops, C, fc, shape, two):
    B, H, W = shape
    gen = torch.Generator().manual_seed(C + H)
    prm = rand_dynca_prm(C, fc, 3, seed=C, scale=2.0)
    x0 = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    cond = torch.rand(B, 3, H, W, generator=gen).to(DEV)
    Tn = 3
    us = torch.rand(Tn, B, 1, H, W, generator=gen).to(DEV)
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    w = dyn_w(ops, prm, x0)
    for rate in (0.5, 0.3):
        bits = ops.pack_fire_mask(us, rate, "dynca")
        o1, s1 = ops.dynca_nsteps(x0, Tn, cond, us, w, "circular", rate, keep_history=True, two_scale=two)
        o2, s2 = ops.dynca_nsteps(x0, Tn, cond, bits, w, "circular", rate, keep_history=True, two_scale=two)
        assert torch.equal(s1, s2)
        g1 = ops.dynca_nsteps_backward(s1, cond, us, w, cot, None, Tn, "circular", rate, two_scale=two)
        g2 = ops.dynca_nsteps_backward(s2, cond, bits, w, cot, None, Tn, "circular", rate, two_scale=two)
        for k in g1:
            assert torch.equal(g1[k], g2[k]), k
