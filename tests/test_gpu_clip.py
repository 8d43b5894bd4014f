"""GPU tests of clip stylisation (csrc/nca_clip.hip, ncahip_dynca_clip_f32, ncahip.video.stylize_clip): the frame front end against
float64, the image output bit for bit, the driver's bookkeeping bit for bit against a Python loop over the same entry points,
continuation, stylize_clip against synthesize_video and a float64 evaluation of the loop, the reference's grey, error paths."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
LUMA = (0.2989, 0.587, 0.114)
MEAN = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)
# |taps| sum to 24 (Laplacian), inputs within [-1, 1]: a dozen roundings of 2^-24 relative on values <= 24 stay under 1.2e-5; tanh is
# 1-Lipschitz and the device tanhf adds a few ulp.  Absolute, with and without tanh.
COND_TOL = 2e-5


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o


def _bank():
    return torch.tensor([O.SOBEL_X, O.SOBEL_Y, O.LAPLACIAN], dtype=torch.float32).reshape(3, 1, 3, 3)


def _cond64(frames64, weights, tanh):
    """frames64 [F,B,3,H,W] float64 in network range -> float64 cond [F,B,3,H,W]: grey, conv2d(padding=1) with the three filters, tanh."""
    Fn, B, _, H, W = frames64.shape
    g = weights[0] * frames64[:, :, 0] + weights[1] * frames64[:, :, 1] + weights[2] * frames64[:, :, 2]
    out = F.conv2d(g.reshape(Fn * B, 1, H, W), _bank().double(), padding=1).reshape(Fn, B, 3, H, W)
    return torch.tanh(out) if tanh else out


def _frames(fmt, Fn, B, H, W, gen):
    """(device frames in the format, the same frames as float64 [F,B,3,H,W] in network range)"""
    if fmt == "u8":
        u8 = torch.randint(0, 256, (Fn, B, H, W, 3), generator=gen, dtype=torch.uint8)
        u8.view(-1)[:4] = torch.tensor([0, 255, 1, 254], dtype=torch.uint8)          # both ends of the range (every shape has >= 6 bytes)
        return u8.to(DEV), (u8.double() / 255.0 * 2.0 - 1.0).permute(0, 1, 4, 2, 3).contiguous()
    f = torch.rand(Fn, B, 3, H, W, generator=gen) * 2 - 1
    return f.to(DEV), f.double()


# ------------------------------------------------------------------ 1. front end against float64
@pytest.mark.parametrize("fmt", ["f32", "u8"])
@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (2, 1, 1, 1), (2, 1, 16, 16), (1, 1, 3, 33), (2, 1, 32, 48)])
def test_clip_cond_against_float64(ops, shape, fmt):
    Fn, B, H, W = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    frames, f64 = _frames(fmt, Fn, B, H, W, gen)
    for gray, wts in (("mean", MEAN), ("luma", LUMA)):
        for tanh in (True, False):
            got = ops.clip_cond(frames, _bank(), gray, tanh)
            assert got.shape == (Fn, B, 3, H, W) and got.dtype == torch.float32
            err = float((got.cpu().double() - _cond64(f64, wts, tanh)).abs().max())
            print(f"clip_cond {shape} {fmt} {gray} tanh={tanh}: max abs err {err:.3e}")
            assert err <= COND_TOL, (shape, fmt, gray, tanh, err)
    ops.check_errors()


def test_clip_cond_unaligned_uint8_views(ops):
    """uint8 frames whose rows start at every byte phase (W * 3 not a multiple of 4, a tensor offset by one byte): the aligned
    4-byte loads of the kernel must pick the same pixels."""
    gen = torch.Generator().manual_seed(3)
    Fn, B, H, W = 2, 1, 6, 67
    buf = torch.randint(0, 256, (Fn * B * H * W * 3 + 1,), generator=gen, dtype=torch.uint8).to(DEV)
    frames = buf[1:].view(Fn, B, H, W, 3)                      # data pointer is odd
    assert frames.data_ptr() % 4 != 0 and frames.is_contiguous()
    f64 = (frames.cpu().double() / 255.0 * 2.0 - 1.0).permute(0, 1, 4, 2, 3).contiguous()
    got = ops.clip_cond(frames, _bank(), "luma", True)
    assert float((got.cpu().double() - _cond64(f64, LUMA, True)).abs().max()) <= COND_TOL
    ops.check_errors()


# ------------------------------------------------------------------ 2. back end, exact
@pytest.mark.parametrize("B,C,c_out,H,W", [(2, 12, 3, 5, 7), (1, 16, 4, 16, 16), (1, 12, 1, 3, 33)])
def test_clip_emit_is_exact(ops, B, C, c_out, H, W):
    gen = torch.Generator().manual_seed(C + W)
    x = torch.rand(B, C, H, W, generator=gen) * 2.4 - 1.2          # beyond +-0.5 on both sides
    special = torch.tensor([0.5, -0.5, 0.0, -0.0, 0.75, -0.75, 0.49999997, -0.49999997, 0.25, 1e-30, -1e-30, 3.0, -3.0])
    n = min(special.numel(), H * W)
    for c in range(c_out):
        x[:, c].reshape(B, -1)[:, :n] = special.roll(c)[:n]
    x = x.to(DEV)
    want = (2 * x[:, :c_out]).clamp(-1, 1).add(1).div(2)
    got = ops.clip_emit(x, c_out)
    assert got.shape == (B, c_out, H, W) and torch.equal(got, want)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))          # the sign of a zero included
    got8 = ops.clip_emit(x, c_out, torch.uint8)
    want8 = (want * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert got8.shape == (B, H, W, c_out) and got8.dtype == torch.uint8 and torch.equal(got8, want8)
    assert int(want8.min()) == 0 and int(want8.max()) == 255
    ops.check_errors()


# ------------------------------------------------------------------ 3. driver, teacher-forced, bit-exact
def _prm(C, fc, seed):
    g = torch.Generator().manual_seed(seed)
    k1 = 4 * C + 3
    return (torch.randn(fc, k1, 1, 1, generator=g) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=g) * 0.1,
            torch.randn(C, fc, 1, 1, generator=g) * (0.6 / fc ** 0.5), torch.randn(C, generator=g) * 0.02)


def _loop(ops, x, cond, us, w, k, step_n, c_out, pad, seed, step0, two):
    """The Python loop the driver replaces: one ops.dynca_nsteps per (frame, k) with that call's masks / Philox steps, then clip_emit."""
    h, f32s, u8s = x, [], []
    for n in range(cond.shape[0] * k):
        un = None if us is None else us[n * step_n:(n + 1) * step_n]
        h, _ = ops.dynca_nsteps(h, step_n, cond[n // k], un, w, pad, 0.5, seed=seed, step0=step0 + n * step_n, two_scale=two)
        h = h.clone()
        f32s.append(ops.clip_emit(h, c_out))
        u8s.append(ops.clip_emit(h, c_out, torch.uint8))
    return torch.stack(f32s), torch.stack(u8s), h


CASES = [(12, 96, 1, 32, 48, False, True), (12, 96, 1, 32, 48, True, True),          # persistent route
         (12, 96, 1, 24, 40, False, False), (12, 96, 1, 24, 40, True, False),        # not a multiple of 16: per-step route
         (32, 256, 1, 16, 16, False, False),                                         # wide: sliced kernels
         (12, 96, 2, 16, 16, False, True)]


@pytest.mark.parametrize("C,fc,B,H,W,two,persistent", CASES)
def test_dynca_clip_equals_the_python_loop_bit_for_bit(ops, C, fc, B, H, W, two, persistent):
    Fn, k, c_out, pad, seed, step0 = 3, 2, 3, "circular", 77, 5
    gen = torch.Generator().manual_seed(C + H + two)
    frames = (torch.rand(Fn, B, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    cond = ops.clip_cond(frames, _bank(), "mean", True)
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    w = ops.DyncaWeights(*_prm(C, fc, C + fc), x)
    assert (ops.lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, 3) > 0) == persistent
    modes = ["bits", "philox"] + (["u"] if (H, two) == (32, False) else [])
    for step_n in (4, 3):                     # odd: the slot that holds the state flips between calls
        for mode in modes:
            us = None
            if mode != "philox":
                us = torch.rand(Fn * k * step_n, B, 1, H, W, generator=gen).to(DEV)
                if mode == "bits":
                    us = ops.pack_fire_mask(us, 0.5, "dynca")
            out_dtype = torch.float32 if step_n == 4 else torch.uint8
            ops.persistent_steps = True
            want32, want8, want_h = _loop(ops, x, cond, us, w, k, step_n, c_out, pad, seed, step0, two)
            want = want32 if out_dtype == torch.float32 else want8
            imgs, h = ops.dynca_clip(x, cond, us, w, k, step_n, c_out, pad, 0.5, seed, step0, two_scale=two, out_dtype=out_dtype)
            tag = (C, fc, B, H, W, two, step_n, mode)
            assert imgs.shape == want.shape and imgs.dtype == out_dtype, tag
            for n in range(Fn * k):
                assert torch.equal(imgs[n], want[n]), (tag, "image", n)
            assert torch.equal(h, want_h), (tag, "state")
            # the other route of the library gives the same bits (persistent launches <-> per-step launches)
            ops.persistent_steps = False
            imgs2, h2 = ops.dynca_clip(x, cond, us, w, k, step_n, c_out, pad, 0.5, seed, step0, two_scale=two, out_dtype=out_dtype)
            ops.persistent_steps = True
            assert torch.equal(imgs2, imgs) and torch.equal(h2, h), (tag, "persistent_steps off")
    assert not torch.equal(want32[0], want32[-1])
    ops.check_errors()


# ------------------------------------------------------------------ 4. continuation
@pytest.mark.parametrize("mode", ["bits", "philox"])
@pytest.mark.parametrize("H,W", [(32, 48), (24, 40)])
def test_dynca_clip_continues_across_calls(ops, mode, H, W):
    Fn, k, step_n, C, fc, seed, step0 = 4, 2, 3, 12, 96, 9, 100
    gen = torch.Generator().manual_seed(H + len(mode))
    frames = (torch.rand(Fn, 1, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    cond = ops.clip_cond(frames, _bank(), "mean", True)
    x = (torch.rand(1, C, H, W, generator=gen) - 0.5).to(DEV)
    w = ops.DyncaWeights(*_prm(C, fc, 4), x)
    us = None
    if mode == "bits":
        us = ops.pack_fire_mask(torch.rand(Fn * k * step_n, 1, 1, H, W, generator=gen).to(DEV), 0.5, "dynca")
    whole, hw = ops.dynca_clip(x, cond, us, w, k, step_n, 3, "replicate", 0.5, seed, step0, two_scale=True)
    half = 2 * k * step_n
    a, ha = ops.dynca_clip(x, cond[:2], None if us is None else us[:half], w, k, step_n, 3, "replicate", 0.5, seed, step0, two_scale=True)
    b, hb = ops.dynca_clip(ha, cond[2:], None if us is None else us[half:], w, k, step_n, 3, "replicate", 0.5, seed, step0 + half, two_scale=True)
    assert torch.equal(torch.cat([a, b]), whole) and torch.equal(hb, hw)
    ops.check_errors()


def _model(scales=(0,), conditioning="edges", C=12, fc=96, seed=0):
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(seed)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning=conditioning, edge_transform="tanh", perception_scales=list(scales),
              device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


@pytest.mark.parametrize("rng", ["torch", "philox"])
@pytest.mark.parametrize("scales", [(0,), (0, 1)])
def test_stylize_clip_does_not_depend_on_frames_per_call(ops, rng, scales):
    from ncahip import video
    m = _model(scales)
    m.mask_rng, m.mask_seed = rng, 11
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (4, 32, 48, 3), generator=gen, dtype=torch.uint8)          # host, decoder-native
    res = []
    for per_call in (32, 1, 3):
        torch.manual_seed(7)
        m._mask_step = 40
        imgs, h = video.stylize_clip(m, frames, step_n=3, steps_per_frame=2, out_dtype=torch.uint8, frames_per_call=per_call)
        assert video.stylize_clip.last_path == "clip" and m._mask_step == 40 + 4 * 2 * 3
        assert imgs.shape == (8, 32, 48, 3) and imgs.dtype == torch.uint8 and imgs.is_cuda and h.shape == (1, 12, 32, 48)
        res.append((imgs, h, torch.cuda.get_rng_state()))
    for imgs, h, st in res[1:]:
        assert torch.equal(imgs, res[0][0]) and torch.equal(h, res[0][1]) and torch.equal(st, res[0][2])
    assert not torch.equal(res[0][0][0], res[0][0][-1])
    ops.check_errors()


# ------------------------------------------------------------------ 5. stylize_clip against the old loop and float64
def test_stylize_clip_luma_against_synthesize_video_and_float64(ops):
    from ncahip import video
    H, W, Fn, k, step_n = 32, 48, 3, 2, 4
    m = _model()
    assert m.mask_rng == "torch"
    gen = torch.Generator().manual_seed(2)
    frames = torch.rand(Fn, 3, H, W, generator=gen) * 2 - 1
    torch.manual_seed(5)
    old = torch.stack(list(video.synthesize_video(m, [f.to(DEV) for f in frames], step_n=step_n, steps_per_frame=k)))
    old_state, old_rng = video.synthesize_video.last_state.clone(), torch.cuda.get_rng_state()
    torch.manual_seed(5)
    new, new_state = video.stylize_clip(m, frames.to(DEV), step_n=step_n, steps_per_frame=k, gray="luma")
    assert video.stylize_clip.last_path == "clip" and new.shape == old.shape == (Fn * k, 3, H, W)
    assert torch.equal(torch.cuda.get_rng_state(), old_rng)                      # the generator ends where the loop leaves it
    # the same masks once more, for the float64 evaluation of the loop (the oracle's DyNCA step, read-only)
    torch.manual_seed(5)
    masks = [ops.unpack_fire_mask(ops.draw_fire_masks(1, H, W, step_n, 0.5, "dynca", DEV), 1, H, W).cpu().double() for _ in range(Fn * k)]
    assert torch.equal(torch.cuda.get_rng_state(), old_rng)
    prm = {n: p.detach().cpu().double() for n, p in m.state_dict().items() if n in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
    h, ref = torch.zeros(1, 12, H, W, dtype=torch.float64), []
    for n in range(Fn * k):
        f64 = frames[n // k].double()
        cond = O.edge_extractor((LUMA[0] * f64[0] + LUMA[1] * f64[1] + LUMA[2] * f64[2])[None, None], "tanh")
        h = O.dynca_nsteps(h, cond, [mk * 0.5 for mk in masks[n]], prm, "circular", 0.5)        # floor(0.5 m + 0.5) = m
        ref.append((O.dynca_to_rgb(h, 3)[0].clamp(-1, 1) + 1) / 2)
    ref = torch.stack(ref)
    e_old, e_new = float((old.cpu().double() - ref).abs().max()), float((new.cpu().double() - ref).abs().max())
    diff = float((old.cpu().double() - new.cpu().double()).abs().max())
    sdiff = float((old_state - new_state).abs().max())
    print(f"stylize_clip vs float64: old loop {e_old:.3e}, clip route {e_new:.3e}; old vs clip {diff:.3e} (final state {sdiff:.3e})")
    assert float(ref.std()) > 1e-3                                               # the images have content
    # two independent fp32 orderings of the same sums: the clip route may be at most twice as far from float64 as the old loop
    assert e_new <= 2 * e_old + 1e-6, (e_old, e_new)
    assert diff <= e_old + e_new + 1e-12                                         # hence the two routes agree (triangle inequality)
    ops.check_errors()


# ------------------------------------------------------------------ 6. the reference's grey
def test_gray_mean_reproduces_the_reference_conditioning(ops):
    from ncahip import video
    m = _model()
    gen = torch.Generator().manual_seed(4)
    frames = torch.rand(2, 3, 32, 48, generator=gen) * 2 - 1
    frames[:, 0] *= 0.2                                                          # unequal channels: mean and luma differ
    bank = torch.cat((m.cond_layer.sobel_x.weight, m.cond_layer.sobel_y.weight, m.cond_layer.laplacian.weight), dim=0)
    mean = ops.clip_cond(frames.to(DEV).unsqueeze(1), bank, "mean", True)[:, 0]
    luma = ops.clip_cond(frames.to(DEV).unsqueeze(1), bank, "luma", True)[:, 0]
    want = O.edge_extractor(frames.double().mean(1, keepdim=True), "tanh")       # EdgeExtractor(RGBToGrayscale(frame)), float64
    assert float((mean.cpu().double() - want).abs().max()) <= COND_TOL
    assert float((mean.cpu().double() - m.cond_layer(frames.to(DEV).mean(1, keepdim=True)).cpu().double()).abs().max()) <= 2 * COND_TOL
    assert float((mean - luma).abs().max()) > 1e-2
    # and it is what stylize_clip conditions on by default: the first image differs between the two greys
    m.mask_rng = "philox"
    m._mask_step = 0
    a, _ = video.stylize_clip(m, frames, step_n=4)
    m._mask_step = 0
    b, _ = video.stylize_clip(m, frames, step_n=4, gray="mean")
    m._mask_step = 0
    c, _ = video.stylize_clip(m, frames, step_n=4, gray="luma")
    assert torch.equal(a, b) and not torch.equal(a, c)
    ops.check_errors()


# ------------------------------------------------------------------ 7. error paths
def test_sticky_error_word_refuses_the_clip(ops):
    from ncahip._capi import NcaHipError
    gen = torch.Generator().manual_seed(6)
    x = (torch.rand(1, 12, 32, 48, generator=gen) - 0.5).to(DEV)
    cond = ops.clip_cond((torch.rand(2, 1, 3, 32, 48, generator=gen) * 2 - 1).to(DEV), _bank(), "mean", True)
    w = ops.DyncaWeights(*_prm(12, 96, 1), x)
    ops.check_errors()
    assert ops.lib().ncahip_debug_inject_error(1) == 0
    try:
        for persist in (True, False):
            ops.persistent_steps = persist
            with pytest.raises(NcaHipError, match="device-side failure"):
                ops.dynca_clip(x, cond, None, w, 1, 4)
    finally:
        ops.persistent_steps = True
        ops.lib().ncahip_check_errors(ops._stream(), 1)      # never leave the word set for later tests
    ops.check_errors()
    imgs, _ = ops.dynca_clip(x, cond, None, w, 1, 4)
    assert bool(torch.isfinite(imgs).all())


def test_unsupported_models_take_the_loop(ops):
    from ncahip import video
    gen = torch.Generator().manual_seed(8)
    frames = torch.rand(2, 3, 32, 48, generator=gen) * 2 - 1
    m = _model(conditioning="pos_emb")
    imgs, h = video.stylize_clip(m, frames, step_n=2, steps_per_frame=2)
    assert video.stylize_clip.last_path == "loop" and imgs.shape == (4, 3, 32, 48) and h.shape == (1, 12, 32, 48)
    m3 = _model(scales=(0, 1, 2))
    imgs, _ = video.stylize_clip(m3, frames, step_n=2, out_dtype=torch.uint8)
    assert video.stylize_clip.last_path == "loop" and imgs.shape == (2, 32, 48, 3) and imgs.dtype == torch.uint8
    m16 = _model()
    video.stylize_clip(m16, frames, step_n=2, state=torch.zeros(1, 12, 32, 48, device=DEV, dtype=torch.bfloat16))
    assert video.stylize_clip.last_path == "loop"
    video.stylize_clip(m16, frames, step_n=2)
    assert video.stylize_clip.last_path == "clip"
    ops.check_errors()
