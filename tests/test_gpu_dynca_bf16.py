"""GPU tests of the opt-in bf16-MFMA DyNCA step (ops.dynca_precision('bf16'), ncahip_dynca_precision mode 1).

Reference and caps: test_dynca_bf16_host.py (the float64 restatement of the contract, the first-order bound E, caps (a) and (b)).
Kernels under test: the DyncaFwdBf / DyncaFwdMsBf variants of dynca_step_fwd_kernel (csrc/nca_dynca_step.h; vector and any-shape form, single- and two-scale) through
ops.dynca_nsteps(keep_history=True); dynca_persist_kernel / dynca_persist_ms_kernel through ops.dynca_nsteps with
ops.persistent_steps; the clip drivers through ncahip.video.stylize_clip(precision='bf16').  Every test prints its figures (-s)."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_dynca_bf16_host import bf16_inputs, check_caps, contract_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
PHILOX_SEED, PHILOX_STEP0 = 0x5EED0002, 9


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        assert o.set_dynca_precision("f32") == "f32"          # every test left the mode as it found it


def _weights(ops, prm, x):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x)


def _one_step(ops, x, cond, u, w, pad, two, philox):
    """one step of the per-step kernels (keep_history: never the persistent kernel), ambient precision; returns (x', u used)"""
    B, _, H, W = x.shape
    if philox:
        u = ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0, device=x.device)
        out, _ = ops.dynca_nsteps(x, 1, cond, None, w, pad, 0.5, seed=PHILOX_SEED, step0=PHILOX_STEP0, keep_history=True, two_scale=two)
    else:
        out, _ = ops.dynca_nsteps(x, 1, cond, u[None], w, pad, 0.5, keep_history=True, two_scale=two)
    return out.clone(), u


#          C   fc  c_cond  B  H   W
SINGLE = [(12, 96, 3, 1, 16, 16),
          (16, 128, 3, 2, 32, 48),
          (13, 96, 2, 1, 24, 40),      # odd C, padded K
          (12, 96, 0, 1, 5, 20),       # smaller than a tile, no conditioning
          (12, 96, 0, 1, 5, 21),       # W % 4 != 0: the any-shape (non-vector) form of the kernel
          (8, 32, 3, 1, 8, 16)]
SINGLE_PADS = [(c, p) for c in SINGLE for p in ("replicate", "circular")] + [(SINGLE[2], "reflect")]
TWO = [((12, 96, 3, 1, 16, 32), "replicate"), ((12, 96, 3, 1, 16, 32), "circular"), ((16, 128, 3, 2, 32, 48), "replicate"),
       ((16, 128, 3, 2, 32, 48), "circular"), ((12, 96, 3, 1, 8, 8), "reflect")]


def _step_case(ops, case, pad, two):
    C, fc, cc, B, H, W = case
    prm, x, cond, u = bf16_inputs(C, fc, cc, B, H, W, seed=1000 * C + H + W + two, device=DEV)
    w = _weights(ops, prm, x)
    scales = (0, 1) if two else (0,)
    exact = O.dynca_step(x, cond, u, prm, pad, 0.5, scales)
    for philox in (False, True):
        with ops.dynca_precision("bf16"):
            got, uu = _one_step(ops, x, cond, u, w, pad, two, philox)
        ref, E = contract_step(x, cond, uu, prm, pad, scales=scales)
        assert 0.25 < float((E > 0).double().mean()) < 0.75 and float(E.max()) > 1e-4        # about half the cells fire; E is not vacuous
        check_caps(got, ref, E, x, f"{case} {pad} two_scale={two} {'philox' if philox else 'explicit u'}")
        if not philox:      # closeness to the exact step: the oracle's fp32 DyNCA step on the same inputs, every element within E
            r = float(((got.double() - exact.double()).abs() / E.clamp_min(1e-30))[E > 0].max())
            print(f"   |bf16 step - exact fp32 oracle step| / E: {r:.3f}")
            assert bool(((got.double() - exact.double()).abs() <= E).all()), r
            f32, _ = _one_step(ops, x, cond, u, w, pad, two, False)                            # and the mode really changes the arithmetic
            assert not torch.equal(f32, got)
            assert float((f32.double() - exact.double()).abs().max()) < 1e-5
    ops.check_errors()


@pytest.mark.parametrize("case,pad", SINGLE_PADS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_single_step_against_the_restatement(ops, case, pad):
    _step_case(ops, case, pad, False)


@pytest.mark.parametrize("case,pad", TWO, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_two_scale_step_against_the_restatement(ops, case, pad):
    _step_case(ops, case, pad, True)


@pytest.mark.parametrize("two", [False, True], ids=["single", "two_scale"])
def test_teacher_forced_replay(ops, two):
    """T = 6 kept states under 'bf16': every stored step against the restatement applied to the kernel's own previous state"""
    C, fc, cc, B, H, W, T = 12, 96, 3, 1, 32, 48, 6
    prm, x, cond, _ = bf16_inputs(C, fc, cc, B, H, W, seed=61 + two, device=DEV)
    us = torch.rand(T, B, 1, H, W, generator=torch.Generator().manual_seed(62)).to(DEV)
    w = _weights(ops, prm, x)
    with ops.dynca_precision("bf16"):
        out, states = ops.dynca_nsteps(x, T, cond, us, w, "circular", 0.5, keep_history=True, two_scale=two)
    assert states.shape[0] == T + 1 and torch.equal(states[0], x) and torch.equal(states[T], out)
    for t in range(T):
        ref, E = contract_step(states[t], cond, us[t], prm, "circular", scales=(0, 1) if two else (0,))
        check_caps(states[t + 1], ref, E, states[t], f"replay step {t} two_scale={two}")
    ops.check_errors()


@pytest.mark.parametrize("two", [False, True], ids=["single", "two_scale"])
@pytest.mark.parametrize("C,fc", [(12, 96), (16, 128)])
@pytest.mark.parametrize("H,W", [(32, 48), (64, 64)])
def test_persistent_equals_per_step_bit_for_bit(ops, H, W, C, fc, two):
    prm, x, cond, _ = bf16_inputs(C, fc, 3, 1, H, W, seed=C + H + two, device=DEV)
    w = _weights(ops, prm, x)
    assert ops.lib().ncahip_dynca_nsteps_persist_workspace(1, C, H, W, fc, 3) > 0
    try:
        for T in (1, 5):
            us = torch.rand(T, 1, 1, H, W, generator=torch.Generator().manual_seed(T)).to(DEV)
            for u_arg in (us, None):
                res = {}
                with ops.dynca_precision("bf16"):
                    for persistent in (True, False):
                        ops.persistent_steps = persistent
                        out, states = ops.dynca_nsteps(x, T, cond, u_arg, w, "replicate", 0.5, seed=PHILOX_SEED, step0=3, two_scale=two)
                        assert (states is None) == persistent          # None: the one-launch kernel took the call
                        res[persistent] = out.clone()
                assert torch.equal(res[True], res[False]), (T, u_arg is None, float((res[True] - res[False]).abs().max()))
                ops.persistent_steps = False
                f32, _ = ops.dynca_nsteps(x, T, cond, u_arg, w, "replicate", 0.5, seed=PHILOX_SEED, step0=3, two_scale=two)
                assert not torch.equal(f32, res[True])
    finally:
        ops.persistent_steps = True
    ops.check_errors()


def _bank():
    return torch.tensor([O.SOBEL_X, O.SOBEL_Y, O.LAPLACIAN], dtype=torch.float32).reshape(3, 1, 3, 3)


def _edge_model(scales):
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(3)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=list(scales),
              device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _extra_model():
    from ncahip.models.dynca_extra import DyNCA
    torch.manual_seed(4)
    m = DyNCA(13, 3, fc_dim=96, padding_mode="circular", pos_emb="CPE", perception_scales=[0], device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


@pytest.mark.parametrize("kind", ["edges", "edges_two_scale", "extra"])
@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_stylize_clip_bf16_equals_the_hand_loop(ops, kind, u8):
    from ncahip import video
    Fn, H, W, step_n = 5, 32, 48, 3
    m = _extra_model() if kind == "extra" else _edge_model((0, 1) if kind == "edges_two_scale" else (0,))
    two = kind == "edges_two_scale"
    m.mask_rng, m.mask_seed = "philox", 11
    gen = torch.Generator().manual_seed(5)
    if u8:
        frames = torch.randint(0, 256, (Fn, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)
    else:
        frames = (torch.rand(Fn, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    out_dtype = torch.uint8 if u8 else torch.float32
    res = {}
    for precision in ("bf16", "f32"):
        m._mask_step = 40
        imgs, h = video.stylize_clip(m, frames, step_n=step_n, out_dtype=out_dtype, precision=precision)
        assert video.stylize_clip.last_path == "clip" and m._mask_step == 40 + Fn * step_n
        assert ops.set_dynca_precision("f32") == "f32"                       # the process mode is what it was before
        res[precision] = (imgs.clone(), h.clone())
    assert not torch.equal(res["bf16"][1], res["f32"][1])
    # the hand loop over ops.dynca_nsteps under the context manager, the same Philox masks
    w = ops.DyncaWeights(m.w1.weight, m.w1.bias, m.w2.weight, m.w2.bias, frames)
    h = m.seed(1, size=(W, H))
    want = []
    with ops.dynca_precision("bf16"):
        if kind == "extra":
            gray = ops.clip_gray(frames.unsqueeze(1), "mean")
            pos = m._cond(h.new_empty(1, m.c_in, H, W))
        else:
            cond = ops.clip_cond(frames.unsqueeze(1), _bank(), "mean", True)
        for n in range(Fn):
            if kind == "extra":
                x, _ = ops.dynca_nsteps(torch.cat((h, gray[n][:, None]), 1), step_n, pos, None, w, "circular", 0.5, seed=11, step0=40 + n * step_n)
                h = x[:, :-1].contiguous()
            else:
                x, _ = ops.dynca_nsteps(h, step_n, cond[n], None, w, "circular", 0.5, seed=11, step0=40 + n * step_n, two_scale=two)
                h = x.clone()
            want.append(ops.clip_emit(x, 3, out_dtype))
    want = torch.cat(want)
    assert res["bf16"][0].shape == want.shape and torch.equal(res["bf16"][0], want) and torch.equal(res["bf16"][1], h)
    ops.check_errors()


def test_loop_route_takes_the_precision_too(ops):
    """a model the clip driver does not cover (positional conditioning on the edge family): the Python loop, same arithmetic switch"""
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(6)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="pos_emb", edge_transform="tanh", perception_scales=[0], device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 3
    frames = (torch.rand(2, 3, 32, 48, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(DEV)
    res = {}
    for precision in ("f32", "bf16"):
        m._mask_step = 0
        imgs, h = video.stylize_clip(m, frames, step_n=2, precision=precision)
        assert video.stylize_clip.last_path == "loop" and ops.set_dynca_precision("f32") == "f32"
        res[precision] = h.clone()
    m._mask_step = 0
    with ops.dynca_precision("bf16"):
        _, want = video.stylize_clip(m, frames, step_n=2)
    assert torch.equal(res["bf16"], want) and not torch.equal(res["bf16"], res["f32"])
    ops.check_errors()


def test_autograd_forward_is_isolated_from_the_mode(ops):
    """a gradient-enabled forward_nsteps inside the context: output and every gradient equal the same call outside it"""
    m = _edge_model((0,))
    m.mask_rng, m.mask_seed = "philox", 5
    g = torch.Generator().manual_seed(9)
    x0 = (torch.rand(1, 12, 32, 48, generator=g) - 0.5).to(DEV)
    img = (torch.rand(1, 1, 32, 48, generator=g) * 2 - 1).to(DEV)
    cot = torch.randn(1, 12, 32, 48, generator=g).to(DEV)

    def run():
        m._mask_step = 0
        m.zero_grad()
        x = x0.clone().requires_grad_(True)
        out, _ = m.forward_nsteps(x, 4, cond_img=img)
        (out * cot).sum().backward()
        return [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in (m.w1.weight, m.w1.bias, m.w2.weight, m.w2.bias)]

    outside = run()
    with ops.dynca_precision("bf16"):
        inside = run()
        with torch.no_grad():                                   # while inference in the same block does run the bf16 step
            m._mask_step = 0
            inf, _ = m.forward_nsteps(x0, 4, cond_img=img)
    for a, b in zip(outside, inside):
        assert torch.equal(a, b)
    assert not torch.equal(inf, outside[0])
    with pytest.raises(RuntimeError):
        with ops.dynca_precision("bf16"):
            raise RuntimeError("inside")
    assert ops.set_dynca_precision("f32") == "f32"
    ops.check_errors()


def test_out_of_range_shapes_ignore_the_mode(ops):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    C, fc, H, W = 20, 96, 16, 32
    assert not ops.dynca_bf16_ok(C, fc)
    prm, x, cond, u = bf16_inputs(C, fc, 3, 1, H, W, seed=20, device=DEV)
    w = _weights(ops, prm, x)
    f32 = ops.dynca_step(x, cond, u, w, "replicate", 0.5)
    assert ops.lib().ncahip_dynca_precision(1) == 0             # at C level: mode 1, the result bit-equal to mode 0
    try:
        bf = ops.dynca_step(x, cond, u, w, "replicate", 0.5)
        bfn, _ = ops.dynca_nsteps(x, 1, cond, u[None], w, "replicate", 0.5)
    finally:
        assert ops.lib().ncahip_dynca_precision(0) == 1
    assert torch.equal(f32, bf) and torch.equal(f32, bfn)
    torch.manual_seed(1)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0], device=torch.device(DEV))
    frames = torch.zeros(2, 3, H, W, device=DEV)
    with pytest.raises(ValueError, match="bf16"):
        video.stylize_clip(m, frames, step_n=2, precision="bf16")
    m12 = _edge_model((0,))
    with pytest.raises(ValueError, match="float32"):
        video.stylize_clip(m12, frames, step_n=2, precision="bf16", state=torch.zeros(1, 12, H, W, device=DEV, dtype=torch.bfloat16))
    assert ops.set_dynca_precision("f32") == "f32"
    ops.check_errors()
