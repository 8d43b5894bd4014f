"""GPU tests of steered DyNCA perception (ncahip_dynca_direction, ops.dynca_direction, DyNCA.forward_nsteps(direction=...),
video.stylize_clip(direction=...)): every forward kernel that rotates the Sobel pair, against a float64 restatement of the steered step.

Kernels under test: dynca_step_fwd_kernel in its variants DyncaFwd / DyncaFwdBf / DyncaFwdMs / DyncaFwdMsBf / DyncaFwdAcc
(csrc/nca_dynca_step.h; tiles 8 x 32) and dynca_persist_kernel / dynca_persist_ms_kernel (csrc/nca_dynca_persist.hip; tiles 16 x 16), all
through ops.dynca_nsteps; the clip drivers through video.stylize_clip; the composed multi-scale step through the model.

The float64 restatement (steered_step64) lives here: F.pad + the four fixed filters, the second scale through F.interpolate, the two
rotation lines, the two 1x1 products, floor(u + rate).  With the identity field it is first held to oracle.nca_oracle's float64 DyNCA
step, exactly.  Bounds are the project's own (tests/util.py): REPLAY_TOL for one step from the same input, REL_TOL for three
free-running steps, both relative to max(1, max|ref|).  Every test prints its measured errors next to the bounds (-s)."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_dynca_bf16_host import bf16_inputs, check_caps, contract_step
from test_gpu_configs import rand_dynca_prm
from util import REL_TOL, REPLAY_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
PADS = ("constant", "replicate", "circular", "reflect")

#        id           C   fc   c_cond B  H   W      reaches
CASES = {"vec":        (12, 96, 3, 2, 10, 36),     # <12,96> VEC, remainder rows and columns, Bd = 1 and Bd = 2
         "any":        (16, 128, 2, 1, 9, 13),     # <16,128> any-shape
         "wide":       (20, 100, 0, 1, 9, 36),     # <32,128>
         "slices":     (12, 192, 2, 1, 8, 32),     # first slice + DyncaFwdAcc
         "ms":         (12, 96, 3, 2, 10, 36),     # two-scale per-step
         "persist":    (12, 96, 3, 1, 32, 32),     # one launch: four tiles, every tile has neighbours
         "persist_ms": (16, 128, 2, 1, 32, 32)}    # likewise, two-scale
TWO_SCALE = ("ms", "persist_ms")
PERSIST = ("persist", "persist_ms")
BF16_IDS = ("vec", "any", "ms", "persist", "persist_ms")          # C <= 16 and fc <= 128: the classes ops.dynca_precision('bf16') covers
ALL_PADS = ("vec", "any", "ms")
T_FREE = 3


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        assert o.set_dynca_precision("f32") == "f32"
        assert o.lib().ncahip_dynca_direction(None, 0, 0, 0) == 0


# ------------------------------------------------------------------ inputs and fields (built once per case, never written to)
@functools.lru_cache(maxsize=None)
def _case(cid):
    """random weights (rand_dynca_prm), a non-zero state, tanh'd conditioning, four steps of explicit uniforms on a 2^-12 grid (so that
    floor(u + 0.5) is the same number in fp32 and float64)"""
    C, fc, cc, B, H, W = CASES[cid]
    seed = 4000 + 17 * sorted(CASES).index(cid)
    prm = {k: v.to(DEV) for k, v in rand_dynca_prm(C, fc, cc, seed).items()}
    g = torch.Generator().manual_seed(seed + 1)
    x = (torch.rand(B, C, H, W, generator=g) * 2 - 1).to(DEV)
    cond = torch.tanh(torch.randn(B, cc, H, W, generator=g) * 2).to(DEV) if cc else None
    us = (torch.floor(torch.rand(4, B, 1, H, W, generator=g) * 4096) / 4096).to(DEV)
    return prm, x, cond, us


@functools.lru_cache(maxsize=None)
def _field(cid, kind):
    """'identity' / 'polar30' / 'uniform40': [1,2,H,W] from ncahip.steer; 'random': [B,2,H,W], non-unit, a field of its own per sample"""
    from ncahip import steer
    _, _, _, B, H, W = CASES[cid]
    if kind == "random":
        g = torch.Generator().manual_seed(99 + sorted(CASES).index(cid))
        return (torch.randn(B, 2, H, W, generator=g) * 0.8).to(DEV).contiguous()
    alignment, angle = {"identity": ("cartesian", 0.0), "polar30": ("polar", 30.0), "uniform40": ("cartesian", 40.0)}[kind]
    return steer.direction_field(alignment, angle, H, W, DEV)


def _weights(ops, prm, x):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x)


def _run(ops, cid, T, dirs=None, pad="replicate", persistent=None, prm=None, inputs=None):
    """T steps of case cid through ops.dynca_nsteps: the per-step kernels, or (PERSIST ids, persistent=None) the one-launch kernel"""
    p0, x, cond, us = inputs if inputs is not None else _case(cid)
    prm = p0 if prm is None else prm
    persistent = (cid in PERSIST) if persistent is None else persistent
    ops.persistent_steps = persistent
    try:
        with ops.dynca_direction(dirs) if dirs is not None else contextlib.nullcontext():
            out, states = ops.dynca_nsteps(x, T, cond, us[:T], _weights(ops, prm, x), pad, 0.5, two_scale=cid in TWO_SCALE)
    finally:
        ops.persistent_steps = True
    assert (states is None) == persistent, (cid, "the one-launch kernel did not take the call" if persistent else "unexpected route")
    return out.clone()


# ------------------------------------------------------------------ the float64 restatement
_FILTERS = ([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], O.SOBEL_X, O.SOBEL_Y, O.LAPLACIAN)


def _perceive64(z, pad):
    """[id | Sx | Sy | L] of z: F.pad(mode) + the four fixed 3 x 3 filters as grouped convolutions"""
    c = z.shape[1]
    zp = F.pad(z, [1, 1, 1, 1], pad)
    return torch.cat([F.conv2d(zp, torch.tensor(f, dtype=z.dtype, device=z.device).reshape(1, 1, 3, 3).repeat(c, 1, 1, 1), groups=c)
                      for f in _FILTERS], dim=1)


def _rotate64(y, dirs, C):
    s, c = dirs[:, 0:1].to(y.dtype), dirs[:, 1:2].to(y.dtype)
    sx, sy = y[:, C:2 * C], y[:, 2 * C:3 * C]
    return torch.cat((y[:, :C], c * sx - s * sy, s * sx + c * sy, y[:, 3 * C:]), dim=1)


def steered_step64(x, cond, u, prm, pad, dirs, scales=(0,), rate=0.5):
    """one steered step in float64; x, cond, u, dirs, prm: any float dtype, on one device"""
    x = x.double()
    B, C, H, W = x.shape
    y = 0
    for s in scales:
        if s == 0:
            y = y + _perceive64(x, pad)
        else:
            xs = F.interpolate(x, size=(H // 2 ** s, W // 2 ** s), mode="bilinear", align_corners=False)
            y = y + F.interpolate(_perceive64(xs, pad), size=(H, W), mode="bilinear", align_corners=False)
    y = _rotate64(y / len(scales), dirs.double(), C)          # the FINAL perception is what turns
    if cond is not None:
        y = torch.cat([y, cond.double()], dim=1)
    w1, b1 = prm["w1.weight"].double().reshape(1, -1, y.shape[1]), prm["w1.bias"].double().reshape(1, -1, 1)
    w2, b2 = prm["w2.weight"].double().reshape(1, C, -1), prm["w2.bias"].double().reshape(1, -1, 1)
    h = F.relu(torch.baddbmm(b1, w1.expand(B, -1, -1), y.reshape(B, -1, H * W)))
    dx = torch.baddbmm(b2, w2.expand(B, -1, -1), h).reshape(B, C, H, W)
    return x + dx * (u.double() + rate).floor()


def _scales(cid):
    return (0, 1) if cid in TWO_SCALE else (0,)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("cid", ["vec", "ms", "persist_ms"])
def test_restatement_with_the_identity_field_is_the_oracle(cid, pad):
    """ties steered_step64 to the pinned oracle: identity field -> oracle.nca_oracle.dynca_step in float64, value for value"""
    prm, x, cond, us = _case(cid)
    p64 = {k: v.double() for k, v in prm.items()}
    want = O.dynca_step(x.double(), None if cond is None else cond.double(), us[0].double(), p64, pad, 0.5, _scales(cid))
    got = steered_step64(x, cond, us[0], prm, pad, _field(cid, "identity"), _scales(cid))
    assert got.dtype == torch.float64 and torch.equal(got, want), float((got - want).abs().max())
    turned = steered_step64(x, cond, us[0], prm, pad, _field(cid, "polar30"), _scales(cid))
    assert float((turned - want).abs().max()) > 1e-3                # and a real field is a different step


# ------------------------------------------------------------------ 1. identity field == unattached, bit for bit
IDENTITY_CASES = [(cid, "f32") for cid in CASES] + [(cid, "bf16") for cid in BF16_IDS]


@pytest.mark.parametrize("cid,precision", IDENTITY_CASES, ids=[f"{c}-{p}" for c, p in IDENTITY_CASES])
def test_identity_field_equals_the_unattached_call(ops, cid, precision):
    assert precision == "f32" or ops.dynca_bf16_ok(*CASES[cid][:2])
    with ops.dynca_precision(precision):
        plain = _run(ops, cid, 2)
        steered = _run(ops, cid, 2, _field(cid, "identity"))
        turned = _run(ops, cid, 2, _field(cid, "polar30"))
    assert torch.equal(steered, plain), float((steered - plain).abs().max())
    assert not torch.equal(turned, plain)                           # the field is honoured at all
    if precision == "bf16":
        assert not torch.equal(plain, _run(ops, cid, 2))            # and the mode was
    ops.check_errors()


# ------------------------------------------------------------------ 2. against the float64 restatement
REF_CASES = [(cid, pad) for cid in CASES for pad in (PADS if cid in ALL_PADS else ("replicate",))]


@pytest.mark.parametrize("kind", ["polar30", "random"])
@pytest.mark.parametrize("cid,pad", REF_CASES, ids=[f"{c}-{p}" for c, p in REF_CASES])
def test_steered_step_against_float64(ops, cid, pad, kind):
    prm, x, cond, us = _case(cid)
    dirs = _field(cid, kind)
    assert dirs.shape[0] == (CASES[cid][3] if kind == "random" else 1)
    one = _run(ops, cid, 1, dirs, pad)
    ref = steered_step64(x, cond, us[0], prm, pad, dirs, _scales(cid))
    e1 = rel_err(one, ref)
    free = _run(ops, cid, T_FREE, dirs, pad)
    r = x
    for t in range(T_FREE):
        r = steered_step64(r, cond, us[t], prm, pad, dirs, _scales(cid))
    e3 = rel_err(free, r)
    moved = float((ref - x.double()).abs().max())
    print(f"{cid} {pad} {kind}: one step {e1:.2e} (bound {REPLAY_TOL:g}), {T_FREE} free-running steps {e3:.2e} (bound {REL_TOL:g}); "
          f"max |x| {float(r.abs().max()):.3g}, the step moves the state by up to {moved:.3g}")
    assert moved > 1e-2
    assert e1 <= REPLAY_TOL and e3 <= REL_TOL
    ops.check_errors()


# ------------------------------------------------------------------ 3. a uniform field == the unsteered kernel on folded weights
@pytest.mark.parametrize("cid", list(CASES))
def test_uniform_field_matches_folded_weights(ops, cid):
    from ncahip import steer
    prm, x, cond, us = _case(cid)
    folded = dict(prm)
    folded["w1.weight"] = steer.fold_angle(prm["w1.weight"], CASES[cid][0], 40.0)
    a = _run(ops, cid, 1, _field(cid, "uniform40"))
    b = _run(ops, cid, 1, None, prm=folded)
    e = rel_err(a, b)
    print(f"{cid}: field path vs folded weights, one step {e:.2e} (bound {REPLAY_TOL:g})")
    assert e <= REPLAY_TOL and not torch.equal(a, _run(ops, cid, 1))
    ops.check_errors()


# ------------------------------------------------------------------ 4. one launch == per-step launches under the same field, bit for bit
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["polar30", "random"])
@pytest.mark.parametrize("cid", PERSIST)
def test_one_launch_equals_per_step_under_a_field(ops, cid, kind, precision):
    with ops.dynca_precision(precision):
        on = _run(ops, cid, 4, _field(cid, kind), persistent=True)
        off = _run(ops, cid, 4, _field(cid, kind), persistent=False)
    assert torch.equal(on, off), float((on - off).abs().max())
    ops.check_errors()


# ------------------------------------------------------------------ 5. bf16 MFMA under a field: the mode's own reference and caps
@pytest.mark.parametrize("cid", ["vec", "ms", "persist", "persist_ms"])
def test_bf16_mfma_under_a_field(ops, cid, monkeypatch):
    """test_dynca_bf16_host.contract_step -- the float64 restatement of the mode's contract with its first-order bound E -- evaluated on
    the STEERED perception: its perception call is replaced, for this test, by the oracle's own followed by the two rotation lines (the
    rotation runs in fp32 before the operand is rounded); inputs (bf16_inputs) and caps (check_caps) are that module's, unchanged."""
    C, fc, cc, B, H, W = CASES[cid]
    inputs = bf16_inputs(C, fc, cc, B, H, W, seed=300 + C + H, device=DEV)
    prm, x, cond, u = inputs
    dirs = _field(cid, "polar30")
    perceive = O.dynca_perceive_multiscale

    def steered(xd, pad, scales=(0,), cnd=None):
        y = _rotate64(perceive(xd, pad, scales, None), dirs.to(xd.dtype), C)
        return y if cnd is None else torch.cat([y, cnd], dim=1)

    with ops.dynca_precision("bf16"):
        got = _run(ops, cid, 1, dirs, "circular", inputs=(prm, x, cond, u[None]))
        plain = _run(ops, cid, 1, None, "circular", inputs=(prm, x, cond, u[None]))
    unsteered_ref, _ = contract_step(x, cond, u, prm, "circular", scales=_scales(cid))
    monkeypatch.setattr(O, "dynca_perceive_multiscale", steered)
    ref, E = contract_step(x, cond, u, prm, "circular", scales=_scales(cid))
    monkeypatch.undo()
    assert float((ref - unsteered_ref).abs().max()) > 1e-2 and float(E.max()) > 1e-4          # the reference is the steered one; E is not vacuous
    check_caps(got, ref, E, x, f"{cid} bf16 MFMA, polar 30")
    assert not torch.equal(got, plain)
    ops.check_errors()


# ------------------------------------------------------------------ 6. a field per sample: the batch stride
@pytest.mark.parametrize("cid", ["vec", "ms"])
def test_per_sample_field_is_indexed_by_the_sample(ops, cid):
    prm, x, cond, us = _case(cid)
    dirs = _field(cid, "random")
    assert dirs.shape[0] == 2 and not torch.equal(dirs[0], dirs[1])
    both = _run(ops, cid, 2, dirs)
    for b in (0, 1):
        alone = _run(ops, cid, 2, dirs[b:b + 1].contiguous(), inputs=(prm, x[b:b + 1].contiguous(), cond[b:b + 1].contiguous(), us[:, b:b + 1].contiguous()))
        assert torch.equal(both[b:b + 1], alone), (b, float((both[b:b + 1] - alone).abs().max()))
    shared = _run(ops, cid, 2, dirs[:1].contiguous())           # Bd = 1: sample 1 under sample 0's field is something else
    assert torch.equal(shared[:1], both[:1]) and not torch.equal(shared[1:], both[1:])
    ops.check_errors()


def test_attached_field_must_fit_the_call(ops):
    from ncahip._capi import NcaHipError
    prm, x, cond, us = _case("vec")
    w = _weights(ops, prm, x)
    with ops.dynca_direction(_field("persist", "polar30")):                       # 32 x 32 against a 10 x 36 call
        with pytest.raises(NcaHipError, match="direction field"):
            ops.dynca_step(x, cond, us[0], w)
    with ops.dynca_direction(_field("vec", "identity")):
        with pytest.raises(NcaHipError, match="direction field"):                 # bf16 storage does not steer
            ops.dynca_nsteps(x.to(torch.bfloat16), 1, cond, us[:1], w)
    with pytest.raises(ValueError):
        with ops.dynca_direction(_field("vec", "random")[:, :, :, ::2]):          # not contiguous
            pass
    with pytest.raises(TypeError):
        with ops.dynca_direction(_field("vec", "random").double()):
            pass
    assert torch.equal(ops.dynca_step(x, cond, us[0], w), _run(ops, "vec", 1))    # detached again after every block
    ops.check_errors()


# ------------------------------------------------------------------ 7. stylize_clip(direction=...)
def _model(family, scales):
    """an edge-conditioned or an extra-channel model with rand_dynca_prm's weights"""
    if family == "edges":
        from ncahip.models.dynca import DyNCA
        m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=list(scales),
                  device=torch.device(DEV))
    else:
        from ncahip.models.dynca_extra import DyNCA
        m = DyNCA(13, 3, fc_dim=96, padding_mode="circular", pos_emb="CPE", perception_scales=list(scales), device=torch.device(DEV))
    prm = rand_dynca_prm(m.c_in, 96, m.c_cond, 77, scale=2.0)
    with torch.no_grad():
        for name, p in (("w1.weight", m.w1.weight), ("w1.bias", m.w1.bias), ("w2.weight", m.w2.weight), ("w2.bias", m.w2.bias)):
            p.copy_(prm[name])
    m.mask_rng, m.mask_seed = "philox", 21
    return m


@pytest.mark.parametrize("family,scales", [("edges", (0,)), ("edges", (0, 1)), ("extra", (0,))], ids=["edges", "edges_two_scale", "extra"])
def test_stylize_clip_direction_equals_the_loop_over_forward_nsteps(ops, family, scales):
    """images and state of stylize_clip(direction=('polar', 45)) == the Python loop over forward_nsteps(..., direction=...), bit for bit.
    The loop's conditioning is the clip's own front end (ops.clip_cond / ops.clip_gray): the module's front end computes the same map
    in another order of roundings (test_gpu_clip.py, COND_TOL), which is not what this test is about."""
    from ncahip import video
    Fn, H, W, step_n, direction = 3, 32, 32, 3, ("polar", 45.0)
    m = _model(family, scales)
    frames = (torch.rand(Fn, 3, H, W, generator=torch.Generator().manual_seed(12)) * 2 - 1).to(DEV)
    m._mask_step = 40
    imgs, h = video.stylize_clip(m, frames, step_n=step_n, direction=direction)
    assert video.stylize_clip.last_path == "clip" and m._mask_step == 40 + Fn * step_n
    assert ops.lib().ncahip_dynca_direction(None, 0, 0, 0) == 0
    m._mask_step = 40
    plain, _ = video.stylize_clip(m, frames, step_n=step_n)
    assert not torch.equal(plain, imgs)
    # the loop
    m._mask_step = 40
    x = m.seed(1, size=(W, H))
    want = []
    if family == "edges":
        layer = m.cond_layer
        bank = torch.cat((layer.sobel_x.weight, layer.sobel_y.weight, layer.laplacian.weight), dim=0)
        cond = ops.clip_cond(frames.unsqueeze(1), bank, "mean", True)
        module_cond = m._cond
        try:
            for n in range(Fn):
                m._cond = lambda state, img, n=n: cond[n]
                with torch.no_grad():
                    x, rgb = m.forward_nsteps(x, step_n, cond_img=frames[n:n + 1].mean(1, keepdim=True), direction=direction)
                want.append((rgb.clamp(-1.0, 1.0) + 1.0) / 2.0)
        finally:
            m._cond = module_cond
    else:
        gray = ops.clip_gray(frames.unsqueeze(1), "mean")
        for n in range(Fn):
            with torch.no_grad():
                full, rgb = m.forward_nsteps(torch.cat((x, gray[n][:, None]), 1), step_n, direction=direction)
            x = full[:, :-1]
            want.append((rgb.clamp(-1.0, 1.0) + 1.0) / 2.0)
    want = torch.cat(want)
    assert imgs.shape == want.shape and torch.equal(imgs, want), float((imgs - want).abs().max())
    assert torch.equal(h, x)
    assert float(imgs.std()) > 1e-3
    # two calls continued through `state` == one call
    m._mask_step = 40
    a, ha = video.stylize_clip(m, frames[:1], step_n=step_n, direction=direction)
    b, hb = video.stylize_clip(m, frames[1:], step_n=step_n, direction=direction, state=ha)
    assert torch.equal(torch.cat([a, b]), imgs) and torch.equal(hb, h)
    # a field tensor is the same argument
    from ncahip import steer
    m._mask_step = 40
    if family == "edges":
        c, hc = video.stylize_clip(m, frames, step_n=step_n, direction=steer.direction_field("polar", 45.0, H, W, DEV))
        assert torch.equal(c, imgs) and torch.equal(hc, h)
    ops.check_errors()


# ------------------------------------------------------------------ 8. the composed multi-scale route
def test_composed_route_against_float64(ops):
    """perception_scales = [0, 1, 2] runs HIP stencil + torch resampling + library GEMMs; the same two lines in torch on the blended
    perception, against the float64 restatement: one step and three free-running steps"""
    H = W = 16
    m = _model("edges", (0, 1, 2))
    assert m._composed(torch.zeros(1, 12, H, W, device=DEV))
    g = torch.Generator().manual_seed(31)
    x0 = (torch.rand(1, 12, H, W, generator=g) * 2 - 1).to(DEV)
    img = (torch.rand(1, 1, H, W, generator=g) * 2 - 1).to(DEV)
    dirs = (torch.randn(1, 2, H, W, generator=g) * 0.8).to(DEV)
    prm = {k: v.detach() for k, v in m.state_dict().items() if k in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
    cond = m._cond(x0, img)
    with torch.no_grad():
        m._mask_step = 5
        one, _ = m.forward_nsteps(x0, 1, cond_img=img, direction=dirs)
        m._mask_step = 5
        free, _ = m.forward_nsteps(x0, T_FREE, cond_img=img, direction=dirs)
        m._mask_step = 5
        plain, _ = m.forward_nsteps(x0, 1, cond_img=img)
    us = [ops.philox_uniform(1, H, W, m.mask_seed, 5 + t, device=DEV) for t in range(T_FREE)]
    # floor(u + 0.5) must be the same number in fp32 and float64 for the draws used
    assert all(bool(((u + 0.5).floor().double() == (u.double() + 0.5).floor()).all()) for u in us)
    r = x0
    for t in range(T_FREE):
        r = steered_step64(r, cond, us[t], prm, "circular", dirs, (0, 1, 2))
        if t == 0:
            e1 = rel_err(one, r)
    e3 = rel_err(free, r)
    print(f"composed [0, 1, 2] at 16 x 16: one step {e1:.2e} (bound {REPLAY_TOL:g}), {T_FREE} free-running steps {e3:.2e} (bound {REL_TOL:g})")
    assert e1 <= REPLAY_TOL and e3 <= REL_TOL and not torch.equal(one, plain)
    # the identity field is the unsteered composed step
    with torch.no_grad():
        m._mask_step = 5
        ident, _ = m.forward_nsteps(x0, 1, cond_img=img, direction=("cartesian", 0.0))
    assert torch.equal(ident, plain)
    ops.check_errors()
