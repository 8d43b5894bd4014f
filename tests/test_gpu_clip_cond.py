"""GPU tests of clip stylisation with ConditionedNCA models (csrc/nca_encoder.hip, ncahip_clip_emit_unit, ncahip_cond_clip_f32,
ncahip.video.stylize_clip_conditioned): the fused encoder against float64, the image output bit for bit, the driver's bookkeeping bit
for bit against a Python loop over the same entry points, continuation and chunking, the whole function against the module loop, and the
sticky error word."""
import copy

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from util import REL_TOL, T, load, near_threshold, rel_err, sd

pytestmark = pytest.mark.gpu
DEV = "cuda"
ENC_TOL = 1e-5     # the project's bound for this quantity (test_conditioning_front_ends_golden_g7); torch's own fp32 encoder sits at ~3e-7

SHAPES = [(1, 1, 1, 1), (2, 1, 5, 7), (1, 2, 16, 16), (1, 1, 17, 33), (2, 1, 3, 70), (1, 1, 32, 48)]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops() as o:
        yield o


def _encoder(E, ch, seed, bias=None):
    from ncahip.encoder import ImageEncoder
    torch.manual_seed(seed)
    enc = ImageEncoder(E, ch)
    if bias is not None:
        with torch.no_grad():
            enc.embed[0].bias.fill_(bias)
    return enc


def _enc64(enc, frames64):
    """frames64 [F,B,ch,H,W] float64 -> the module's own forward in float64 on the CPU, [F,B,E,H,W]"""
    Fn, B = frames64.shape[:2]
    with torch.no_grad():
        out = copy.deepcopy(enc).cpu().double()(frames64.reshape(Fn * B, *frames64.shape[2:]))
    return out.reshape(Fn, B, *out.shape[1:])


def _frames(fmt, Fn, B, ch, H, W, gen):
    """(device frames in the format, the same frames as float64 [F,B,ch,H,W] in [0, 1])"""
    if fmt == "u8":
        u8 = torch.randint(0, 256, (Fn, B, H, W, 3), generator=gen, dtype=torch.uint8)
        u8.view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)          # both ends of the byte range
        return u8.to(DEV), (u8.double() / 255.0).permute(0, 1, 4, 2, 3).contiguous()
    f = torch.rand(Fn, B, ch, H, W, generator=gen)
    return f.to(DEV), f.double()


# ------------------------------------------------------------------ 1. encoder against float64
@pytest.mark.parametrize("E", [8, 12, 16, 28])
def test_clip_encode_against_float64(ops, E):
    enc = _encoder(E, 3, E)
    for shape in SHAPES:
        for fmt in ("f32", "u8"):
            Fn, B, H, W = shape
            frames, f64 = _frames(fmt, Fn, B, 3, H, W, torch.Generator().manual_seed(H * 100 + W))
            got = ops.clip_encode(frames, enc)
            assert got.shape == (Fn, B, E, H, W)
            err = rel_err(got, _enc64(enc, f64))
            print(f"clip_encode E={E} {fmt} {shape}: rel err {err:.3e}")
            assert err < ENC_TOL, (shape, fmt, err)
    # the zero padding of h1: with a bias of +0.5 everywhere relu(b1 + ...) is far from 0 on the halo, and conv2 must still see zeros there
    encb = _encoder(E, 3, E + 1, bias=0.5)
    for shape in ((1, 1, 1, 1), (2, 1, 5, 7), (1, 1, 17, 33)):
        Fn, B, H, W = shape
        frames, f64 = _frames("f32", Fn, B, 3, H, W, torch.Generator().manual_seed(W))
        err = rel_err(ops.clip_encode(frames, encb), _enc64(encb, f64))
        print(f"clip_encode E={E} bias +0.5 {shape}: rel err {err:.3e}")
        assert err < ENC_TOL, (shape, err)
    ops.check_errors()


@pytest.mark.parametrize("ch,E", [(4, 12), (1, 16)])
def test_clip_encode_other_channel_counts(ops, ch, E):
    enc = _encoder(E, ch, 10 + ch)
    for shape in ((2, 1, 5, 7), (1, 1, 17, 33)):
        Fn, B, H, W = shape
        frames, f64 = _frames("f32", Fn, B, ch, H, W, torch.Generator().manual_seed(H))
        err = rel_err(ops.clip_encode(frames, enc), _enc64(enc, f64))
        print(f"clip_encode ch={ch} E={E} {shape}: rel err {err:.3e}")
        assert err < ENC_TOL, (shape, err)
    ops.check_errors()


def test_clip_encode_golden_g7(ops):
    """The reference-generated G7 fixture: the reference's own ImageEncoder output for its own weights."""
    from ncahip.encoder import ImageEncoder
    g = load("g7_encoders")
    enc = ImageEncoder(8, 3)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd(g).items()}, strict=True)
    img = T(g["img"], DEV)
    got = ops.clip_encode(img.unsqueeze(0), enc)[0]
    err = rel_err(got, T(g["enc_out"]))
    print(f"clip_encode G7: rel err {err:.3e}")
    assert err < ENC_TOL
    # frames and batch are the same axis to the kernel
    assert torch.equal(ops.clip_encode(img.unsqueeze(1), enc)[:, 0], got)


# ------------------------------------------------------------------ 2. uint8 byte phases
def test_clip_encode_unaligned_uint8_views(ops):
    """uint8 frames whose rows start at every byte phase (W * 3 not a multiple of 4, a tensor offset by one byte, more than one tile
    per row): the aligned 4-byte loads must pick the same pixels, and nothing outside the tensor."""
    gen = torch.Generator().manual_seed(3)
    enc = _encoder(12, 3, 5)
    for Fn, B, H, W in ((2, 1, 6, 67), (1, 2, 19, 21)):
        buf = torch.randint(0, 256, (Fn * B * H * W * 3 + 1,), generator=gen, dtype=torch.uint8).to(DEV)
        frames = buf[1:].view(Fn, B, H, W, 3)                      # data pointer is odd
        assert frames.data_ptr() % 4 != 0 and frames.is_contiguous() and (W * 3) % 4 != 0
        f64 = (frames.cpu().double() / 255.0).permute(0, 1, 4, 2, 3).contiguous()
        err = rel_err(ops.clip_encode(frames, enc), _enc64(enc, f64))
        print(f"clip_encode unaligned uint8 {(Fn, B, H, W)}: rel err {err:.3e}")
        assert err < ENC_TOL, err
    ops.check_errors()


# ------------------------------------------------------------------ 3. emit, exact
@pytest.mark.parametrize("B,C,H,W", [(2, 5, 5, 7), (1, 20, 16, 16), (1, 3, 9, 89)])
def test_clip_emit_unit_is_exact(ops, B, C, H, W):
    gen = torch.Generator().manual_seed(C + W)
    one, zero = np.float32(1.0), np.float32(0.0)
    ks = np.arange(256, dtype=np.float32) / np.float32(255.0)                      # the uint8 truncation boundaries k / 255 and their neighbours
    bound = np.concatenate([ks, np.nextafter(ks, np.float32(-1)), np.nextafter(ks, np.float32(2))]).astype(np.float32)
    special = np.array([-0.0, 0.0, 1.0, np.nextafter(zero, -one), np.nextafter(one, np.float32(2)), -1e-30, 1e-30, -3.0, 3.0, 0.5,
                        np.float32(-np.inf), np.float32(np.inf)], dtype=np.float32)
    vals = torch.from_numpy(np.concatenate([special, bound]))
    for out_dtype in (torch.float32, torch.uint8):
        x = torch.rand(B, C, H, W, generator=gen) * 1.6 - 0.3          # beyond [0, 1] on both sides
        v = torch.cat([vals, torch.tensor([float("nan")])]) if out_dtype == torch.float32 else vals
        n = min(v.numel(), H * W)
        for c in range(3):
            x[:, c].reshape(B, -1)[:, :n] = v.roll(7 * c)[:n]
        x = x.to(DEV)
        img = torch.clamp(x[:, :3], 0.0, 1.0)
        got = ops.clip_emit_unit(x, out_dtype)
        if out_dtype == torch.uint8:
            want = (img * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
            assert got.shape == (B, H, W, 3) and torch.equal(got, want)
        else:
            assert got.shape == (B, 3, H, W)
            assert torch.equal(got.view(torch.int32), img.contiguous().view(torch.int32))      # NaN and the sign of a zero included
            assert bool(torch.isnan(got).any())
    ops.check_errors()


# ------------------------------------------------------------------ 4. driver, bit for bit
def _weights(ops, C, seed, like):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    return ops.CondWeights(r(3 * C, 1, 3, 3, k=0.3), r(64, 3 * C, 1, 1, k=0.14), r(64, k=0.1), r(64, 64, 1, 1, k=0.12), r(64, k=0.1),
                           r(C, 64, 1, 1, k=0.04), like)


def _dense_state(B, C, H, W, gen):
    x = torch.rand(B, C, H, W, generator=gen) * 0.8
    x[:, 3] = 1.0                   # alive everywhere: every cell does real work
    return x.to(DEV)


def _hand_loop(ops, x, goal, us, w, k, step_n, seed, step0, out_dtype, same_goal=False):
    """the loop ncahip_cond_clip_f32 replaces, over the same entry points"""
    imgs = []
    for n in range(goal.shape[0] * k):
        un = None if us is None else us[n * step_n:(n + 1) * step_n]
        x, _, _ = ops.cond_grow(x, step_n, goal[0 if same_goal else n // k], un, w, seed=seed, step0=step0 + n * step_n)
        imgs.append(ops.clip_emit_unit(x, out_dtype))
    return torch.stack(imgs), x


@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("B,C,H,W", [(1, 20, 16, 16), (1, 20, 24, 40), (2, 20, 16, 16), (1, 16, 16, 16)])
def test_cond_clip_equals_the_hand_loop(ops, B, C, H, W, persistent):
    """(1, 20, 16, 16) and (1, 16, 16, 16) are covered by the persistent grow, 24 x 40 is not (H % 16), float uniforms never are."""
    ops.persistent_cond = persistent
    gen = torch.Generator().manual_seed(H + W + C + B)
    Fn, E = 3, C - 4
    x0 = _dense_state(B, C, H, W, gen)
    goal = (torch.randn(Fn, B, E, H, W, generator=gen) * 0.5).to(DEV)
    w = _weights(ops, C, C, x0)
    guarded = False
    for step_n in (2, 3):
        for k in (1, 2):
            uf = torch.rand(Fn * k * step_n, B, 1, H, W, generator=gen).to(DEV)
            for masks in ("bits", "philox", "float"):
                us = {"bits": ops.pack_fire_mask(uf, 0.5, "cond"), "philox": None, "float": uf}[masks]
                for out_dtype in (torch.float32, torch.uint8):
                    imgs, xs = ops.cond_clip(x0, goal, us, w, k, step_n, seed=11, step0=5, out_dtype=out_dtype)
                    ref_i, ref_x = _hand_loop(ops, x0, goal, us, w, k, step_n, 11, 5, out_dtype)
                    tag = (step_n, k, masks, out_dtype)
                    assert imgs.shape == ref_i.shape and torch.equal(imgs, ref_i), tag
                    assert torch.equal(xs, ref_x), tag
                    assert not torch.equal(xs, x0), tag
                    if not guarded:       # the goal of every frame matters: frame 0's goal for all frames gives other images
                        oth_i, _ = _hand_loop(ops, x0, goal, us, w, k, step_n, 11, 5, out_dtype, same_goal=True)
                        assert torch.equal(oth_i[:k], ref_i[:k]) and not torch.equal(oth_i[k:], ref_i[k:])
                        guarded = True
    ops.check_errors()


def test_driver_shapes_take_the_routes_they_are_meant_for(ops):
    """The persistent grow accepts the 16 x 16 shapes of the test above on this device and never covers 24 x 40: so that test runs both
    routes of the driver, and the switch from the first NCAHIP_ERANGE on."""
    from ncahip import _capi
    L = _capi.lib()
    assert L.ncahip_cond_grow_persist_workspace(1, 20, 24, 40, 64, 16) == 0
    gen = torch.Generator().manual_seed(1)
    for B, C in ((1, 20), (2, 20), (1, 16)):
        x0 = _dense_state(B, C, 16, 16, gen)
        goal = (torch.randn(B, C - 4, 16, 16, generator=gen) * 0.5).to(DEV)
        w = _weights(ops, C, C, x0)
        nbytes = L.ncahip_cond_grow_persist_workspace(B, C, 16, 16, 64, C - 4)
        assert nbytes > 0
        ws, out = torch.zeros(nbytes, device=DEV, dtype=torch.uint8), torch.empty_like(x0)
        rc = L.ncahip_cond_grow_fwd_persist_f32(x0.data_ptr(), None, 2, 2, out.data_ptr(), goal.data_ptr(), C - 4, None, w.wp.data_ptr(),
                                                w.w1.data_ptr(), w.b1.data_ptr(), w.w2.data_ptr(), w.b2.data_ptr(), w.w3.data_ptr(), B, C, 16, 16,
                                                64, 3, 0.1, 0.5, -10.0, 10.0, 11, 5, ws.data_ptr(), nbytes, 1, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, (B, C, L.ncahip_last_error())
        ops.persistent_cond = False
        ref, _, _ = ops.cond_grow(x0, 2, goal, None, w, seed=11, step0=5)
        assert torch.equal(out, ref)
    ops.check_errors()


# ------------------------------------------------------------------ 5./6. stylize_clip_conditioned
def _model(hidden=16, seed=0, size=16):
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(seed)
    m = ConditionedNCA(target_shape=(3, size, size), num_hidden_channels=hidden)
    with torch.no_grad():
        m.update_net.out[4].weight.mul_(0.3)
    return m.to(DEV)


def _clip_frames(n, H, W, seed, u8=False):
    gen = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)
    return torch.rand(n, 3, H, W, generator=gen).to(DEV)


@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("u8", [False, True])
def test_stylize_clip_conditioned_continuation_and_chunking(ops, u8, persistent):
    from ncahip import video
    ops.persistent_cond = persistent
    m = _model()
    frames = _clip_frames(4, 16, 16, 7, u8)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(1))
    dt = torch.uint8 if u8 else torch.float32

    def run(parts, per_call, rng):
        m.mask_rng, m._mask_step = rng, 0
        torch.manual_seed(123)
        h, outs = x0, []
        for part in parts:
            imgs, h = video.stylize_clip_conditioned(m, part, step_n=3, steps_per_frame=2, state=h, out_dtype=dt, frames_per_call=per_call)
            assert video.stylize_clip_conditioned.last_path == "clip"
            outs.append(imgs)
        return torch.cat(outs), h, torch.cuda.get_rng_state(), m._mask_step

    for rng in ("torch", "philox"):
        base = run([frames], 8, rng)
        assert base[0].shape == ((8, 16, 16, 3) if u8 else (8, 3, 16, 16)) and base[0].dtype == dt and base[3] == 4 * 2 * 3
        for other in (run([frames[:2], frames[2:]], 8, rng), run([frames], 1, rng), run([frames], 3, rng)):
            assert torch.equal(other[0], base[0]) and torch.equal(other[1], base[1])
            assert torch.equal(other[2], base[2]) and other[3] == base[3]
    ops.check_errors()


def test_stylize_clip_conditioned_equals_the_hand_loop_and_seeds(ops):
    """The whole function against the loop of section 4 built from the module's own parameters, masks drawn as ConditionedNCA._draw draws
    them; state=None seeds the grid and warmup_steps run on frame 0's goal before the first image."""
    from ncahip import video
    ops.persistent_cond = False
    m = _model(seed=2)
    frames = _clip_frames(3, 16, 16, 9)
    torch.manual_seed(5)
    m._mask_step = 0
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=4, steps_per_frame=1, warmup_steps=6)
    assert video.stylize_clip_conditioned.last_path == "clip" and imgs.shape == (3, 3, 16, 16) and m._mask_step == 6 + 12
    end = torch.cuda.get_rng_state()
    torch.manual_seed(5)
    goal = ops.clip_encode(frames.unsqueeze(1), m.encoder)
    x = m.generate_seed(1, size=16).to(DEV)
    w = m._weights(x)
    x, _, _ = ops.cond_grow(x, 6, goal[0], m._draw(x, 6), w)
    want = []
    for f in range(3):
        x, _, _ = ops.cond_grow(x, 4, goal[f], m._draw(x, 4), w)
        want.append(ops.clip_emit_unit(x))
    assert torch.equal(imgs, torch.cat(want)) and torch.equal(h, x) and torch.equal(end, torch.cuda.get_rng_state())
    assert float(imgs.max()) > 0.0        # the seed has grown into the image


def test_stylize_clip_conditioned_against_the_module_loop(ops):
    """One frame, step_n = 2, against the loop over nca.grow (front pass + MIOpen encoder) within REL_TOL.  The comparison is continuous
    only if no life mask sits on its threshold: asserted on every state and pending state of the float64 trajectory."""
    from ncahip import video
    ops.persistent_cond = False
    m = _model(seed=4)
    m.mask_rng, m.mask_seed = "philox", 77
    frames = _clip_frames(1, 16, 16, 21)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(8))
    # float64 oracle trajectory
    prm = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    enc64 = copy.deepcopy(m.encoder).cpu().double()
    with torch.no_grad():
        gpad = O.cond_pad_goal(enc64(frames.cpu().double()), 20)
    x = x0.cpu().double()
    for t in range(2):
        u = torch.from_numpy(np.asarray(O.philox_uniform(77, t, 1, 16, 16))).reshape(1, 1, 16, 16)
        r = O.cond_step(x, gpad, u, prm, 3, return_all=True)
        assert not bool(near_threshold(x).any()) and not bool(near_threshold(r["x1"]).any()), t
        x = r["x2"]
    ref64 = torch.clamp(x[:, :3], 0.0, 1.0)
    m._mask_step = 0
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=2, state=x0)
    assert video.stylize_clip_conditioned.last_path == "clip"
    m._mask_step = 0
    with torch.no_grad():
        loop_state = m.grow(x0, 2, frames[0:1])
        loop_img = torch.clamp(loop_state[:, :3], 0.0, 1.0)
    e_img, e_state, e_64 = rel_err(imgs, loop_img), rel_err(h, loop_state), rel_err(imgs, ref64)
    print(f"stylize_clip_conditioned vs module loop: image {e_img:.3e}, state {e_state:.3e}; vs float64 image {e_64:.3e}")
    assert e_img < REL_TOL and e_state < REL_TOL and e_64 < REL_TOL
    assert float((imgs - x0[:, :3].clamp(0, 1)).abs().max()) > 1e-3       # the steps moved the image


class _WrappedEncoder(torch.nn.Module):
    """A custom encoder module: not the class the fused kernel covers."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x) * 0.5


@pytest.mark.parametrize("u8", [False, True])
def test_stylize_clip_conditioned_loop_route(ops, u8):
    from ncahip import video
    from ncahip.nca import ConditionedNCA
    from ncahip.encoder import ImageEncoder
    torch.manual_seed(3)
    m = ConditionedNCA(encoder=_WrappedEncoder(ImageEncoder(16, 3)), target_shape=(3, 16, 16)).to(DEV)
    frames = _clip_frames(2, 16, 16, 4, u8)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(2))
    torch.manual_seed(9)
    m._mask_step = 0
    dt = torch.uint8 if u8 else torch.float32
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=3, steps_per_frame=2, state=x0, out_dtype=dt)
    assert video.stylize_clip_conditioned.last_path == "loop"
    torch.manual_seed(9)
    m._mask_step = 0
    state, want = x0, []
    with torch.no_grad():
        for f in range(2):
            frame = (frames[f].float() / 255.0).permute(2, 0, 1) if u8 else frames[f]
            for _ in range(2):
                state = m.grow(state, 3, frame[None])
                img = torch.clamp(state[:, :3], 0.0, 1.0)
                want.append((img * 255.0).to(torch.uint8).permute(0, 2, 3, 1) if u8 else img)
    assert torch.equal(imgs, torch.cat(want)) and torch.equal(h, state)
    ops.check_errors()


# ------------------------------------------------------------------ 7. sticky error word
@pytest.mark.parametrize("persistent", [True, False])
def test_cond_clip_refuses_on_the_sticky_error_word(ops, persistent):
    from ncahip import _capi
    L = _capi.lib()
    B, C, H, W, E, Fn = 1, 20, 16, 16, 16, 2
    gen = torch.Generator().manual_seed(0)
    w = _weights(ops, C, 1, _dense_state(B, C, H, W, gen))
    states = torch.full((4, B, C, H, W), -7.0, device=DEV)
    states[0] = _dense_state(B, C, H, W, gen)
    before = states.clone()
    pre = torch.full((2, B, H, W), 9, device=DEV, dtype=torch.uint8)
    goal = torch.randn(Fn, B, E, H, W, generator=gen).to(DEV)
    images = torch.full((Fn, B, 3, H, W), -7.0, device=DEV)
    nbytes = L.ncahip_cond_grow_persist_workspace(B, C, H, W, 64, E)
    assert nbytes > 0
    ws = torch.zeros(nbytes, device=DEV, dtype=torch.uint8) if persistent else None
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    assert L.ncahip_debug_inject_error(1) == 0
    try:
        rc = L.ncahip_cond_clip_f32(states.data_ptr(), pre.data_ptr(), goal.data_ptr(), E, images.data_ptr(), _capi.CLIP_F32_NCHW, Fn, 1, 2, None,
                                    w.wp.data_ptr(), w.w1.data_ptr(), w.b1.data_ptr(), w.w2.data_ptr(), w.b2.data_ptr(), w.w3.data_ptr(), B, C, H,
                                    W, 64, 3, 0.1, 0.5, -10.0, 10.0, 0, 0, None if ws is None else ws.data_ptr(), nbytes if persistent else 0, 1,
                                    stream)
        assert rc == _capi.EDEVICE and b"error word" in L.ncahip_last_error()
        torch.cuda.synchronize()
        assert torch.equal(states, before) and bool((images == -7.0).all()) and bool((pre == 9).all())      # nothing was enqueued
        if ws is not None:
            assert int(ws.sum()) == 0
    finally:
        assert L.ncahip_check_errors(stream, 1) == _capi.EDEVICE      # reports it once more and clears it
    assert L.ncahip_check_errors(stream, 0) == 0
    ops.check_errors()
