"""GPU tests of clip stylisation for the extra-channel models (ncahip_clip_gray, ncahip_clip_emit_inject, ncahip_dynca_clip_xc_f32,
ncahip.video.stylize_clip with ncahip.models.dynca_extra.DyNCA): the grey against float64, emit + inject bit for bit, the driver bit for
bit against a Python loop over the existing entry points, continuation and chunking, stylize_clip against the reference's loop
(ExtraChannels/utils/misc/video_utils.py:66-82) and a float64 evaluation of it, routes and error paths."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
LUMA = (0.2989, 0.587, 0.114)
MEAN = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)
# inputs within [-1, 1], weights that sum to 1: at most five roundings of 2^-24 in the weighted sum, two per channel in the uint8 widening
# and the float32 rounding of the weights stay under 5e-7.  Absolute.
GRAY_TOL = 1e-6


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o


def _gray64(frames64, weights):
    """frames64 [F,B,3,H,W] float64 in network range -> float64 grey [F,B,H,W]"""
    return weights[0] * frames64[:, :, 0] + weights[1] * frames64[:, :, 1] + weights[2] * frames64[:, :, 2]


def _frames(fmt, Fn, B, H, W, gen):
    """(device frames in the format, the same frames as float64 [F,B,3,H,W] in network range)"""
    if fmt == "u8":
        u8 = torch.randint(0, 256, (Fn, B, H, W, 3), generator=gen, dtype=torch.uint8)
        u8.view(-1)[:4] = torch.tensor([0, 255, 1, 254], dtype=torch.uint8)          # both ends of the range (every shape has >= 6 bytes)
        return u8.to(DEV), (u8.double() / 255.0 * 2.0 - 1.0).permute(0, 1, 4, 2, 3).contiguous()
    f = torch.rand(Fn, B, 3, H, W, generator=gen) * 2 - 1
    return f.to(DEV), f.double()


# ------------------------------------------------------------------ 1. grey against float64
@pytest.mark.parametrize("fmt", ["f32", "u8"])
@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (2, 1, 1, 1), (2, 1, 16, 16), (1, 1, 3, 33), (2, 1, 32, 48)])
def test_clip_gray_against_float64(ops, shape, fmt):
    Fn, B, H, W = shape
    gen = torch.Generator().manual_seed(H * 100 + W)
    frames, f64 = _frames(fmt, Fn, B, H, W, gen)
    for gray, wts in (("mean", MEAN), ("luma", LUMA)):
        got = ops.clip_gray(frames, gray)
        assert got.shape == (Fn, B, H, W) and got.dtype == torch.float32
        err = float((got.cpu().double() - _gray64(f64, wts)).abs().max())
        print(f"clip_gray {shape} {fmt} {gray}: max abs err {err:.3e}")
        assert err <= GRAY_TOL, (shape, fmt, gray, err)
    ops.check_errors()


def test_clip_gray_unaligned_uint8_views(ops):
    """uint8 frames whose rows start at every byte phase (W * 3 not a multiple of 4, a tensor offset by one byte, more than one tile
    per row): the aligned 4-byte loads must pick the same pixels, and nothing outside the tensor."""
    gen = torch.Generator().manual_seed(3)
    Fn, B, H, W = 2, 1, 6, 67
    buf = torch.randint(0, 256, (Fn * B * H * W * 3 + 1,), generator=gen, dtype=torch.uint8).to(DEV)
    frames = buf[1:].view(Fn, B, H, W, 3)                      # data pointer is odd
    assert frames.data_ptr() % 4 != 0 and frames.is_contiguous()
    f64 = (frames.cpu().double() / 255.0 * 2.0 - 1.0).permute(0, 1, 4, 2, 3).contiguous()
    for gray, wts in (("mean", MEAN), ("luma", LUMA)):
        err = float((ops.clip_gray(frames, gray).cpu().double() - _gray64(f64, wts)).abs().max())
        print(f"clip_gray unaligned uint8 {gray}: max abs err {err:.3e}")
        assert err <= GRAY_TOL, (gray, err)
    ops.check_errors()


# ------------------------------------------------------------------ 2. emit + inject, exact
@pytest.mark.parametrize("B,C,c_out,H,W", [(2, 13, 3, 5, 7), (1, 16, 3, 16, 16), (1, 13, 1, 3, 33), (1, 5, 4, 3, 5)])
def test_clip_emit_inject_is_exact(ops, B, C, c_out, H, W):
    gen = torch.Generator().manual_seed(C + W)
    x = torch.rand(B, C, H, W, generator=gen) * 2.4 - 1.2          # beyond +-0.5 on both sides
    special = torch.tensor([0.5, -0.5, 0.0, -0.0, 0.75, -0.75, 0.49999997, -0.49999997, 0.25, 1e-30, -1e-30, 3.0, -3.0])
    n = min(special.numel(), H * W)
    for c in range(c_out):
        x[:, c].reshape(B, -1)[:, :n] = special.roll(c)[:n]
    x = x.to(DEV)
    plane = (torch.rand(B, H, W, generator=gen) * 2 - 1).to(DEV)
    plane.view(-1)[:2] = torch.tensor([0.0, -0.0], device=DEV)
    for out_dtype in (torch.float32, torch.uint8):
        want = ops.clip_emit(x, c_out, out_dtype)
        bits = (lambda t: t.view(torch.int32)) if out_dtype == torch.float32 else (lambda t: t)      # the sign of a zero included
        # both halves in one launch
        s = x.clone()
        got = ops.clip_emit_inject(s, c_out, plane, out_dtype)
        assert got.shape == want.shape and got.dtype == out_dtype and torch.equal(bits(got), bits(want)), out_dtype
        assert torch.equal(s[:, -1].view(torch.int32), plane.view(torch.int32)) and torch.equal(s[:, :-1], x[:, :-1]), out_dtype
        # emit only: the state is left alone
        s = x.clone()
        got = ops.clip_emit_inject(s, c_out, None, out_dtype)
        assert torch.equal(bits(got), bits(want)) and torch.equal(s.view(torch.int32), x.view(torch.int32)), out_dtype
        # inject only
        s = x.clone()
        assert ops.clip_emit_inject(s, c_out, plane, out_dtype, emit=False) is None
        assert torch.equal(s[:, -1].view(torch.int32), plane.view(torch.int32)) and torch.equal(s[:, :-1], x[:, :-1]), out_dtype
    want8 = ops.clip_emit(x, c_out, torch.uint8)
    assert int(want8.min()) == 0 and int(want8.max()) == 255
    ops.check_errors()


# ------------------------------------------------------------------ 3. driver, teacher-forced, bit-exact
def _prm(C, fc, c_cond, seed):
    g = torch.Generator().manual_seed(seed)
    k1 = 4 * C + c_cond
    return (torch.randn(fc, k1, 1, 1, generator=g) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=g) * 0.1,
            torch.randn(C, fc, 1, 1, generator=g) * (0.6 / fc ** 0.5), torch.randn(C, generator=g) * 0.02)


def _loop(ops, x, gray, cond, us, w, k, step_n, c_out, pad, seed, step0, two, reinject=True):
    """The Python loop the driver replaces, over the existing entry points: x[:, -1] = gray[n // k], one ops.dynca_nsteps with that
    call's masks / Philox steps, then clip_emit.  reinject=False leaves the repeats j > 0 of a frame without their grey (the guard)."""
    h, f32s, u8s = x.clone(), [], []
    for n in range(gray.shape[0] * k):
        if reinject or n % k == 0:
            h[:, -1] = gray[n // k]
        un = None if us is None else us[n * step_n:(n + 1) * step_n]
        h, _ = ops.dynca_nsteps(h, step_n, cond, un, w, pad, 0.5, seed=seed, step0=step0 + n * step_n, two_scale=two)
        h = h.clone()
        f32s.append(ops.clip_emit(h, c_out))
        u8s.append(ops.clip_emit(h, c_out, torch.uint8))
    return torch.stack(f32s), torch.stack(u8s), h


CASES = [(13, 96, 2, 1, 32, 48, False, True), (13, 96, 2, 1, 32, 48, True, True), (16, 128, 2, 1, 32, 48, True, True),      # persistent route
         (13, 96, 0, 1, 32, 48, False, True),                                                # no cond map
         (13, 96, 2, 1, 24, 40, False, False), (13, 96, 2, 1, 24, 40, True, False),          # not a multiple of 16: per-step route
         (13, 96, 2, 2, 16, 16, False, True)]


@pytest.mark.parametrize("C,fc,c_cond,B,H,W,two,persistent", CASES)
def test_dynca_clip_xc_equals_the_python_loop_bit_for_bit(ops, C, fc, c_cond, B, H, W, two, persistent):
    Fn, k, c_out, pad, seed, step0 = 3, 2, 3, "circular", 77, 5
    gen = torch.Generator().manual_seed(C + H + two + c_cond)
    frames = (torch.rand(Fn, B, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    gray = ops.clip_gray(frames, "mean")
    cond = O.cpe2d(B, H, W).to(DEV) if c_cond else None
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    w = ops.DyncaWeights(*_prm(C, fc, c_cond, C + fc), x)
    assert (ops.lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, c_cond) > 0) == persistent
    modes = ["bits", "philox"] + (["u"] if (H, two, c_cond, B) == (32, False, 2, 1) else [])
    for step_n in (4, 3):                     # odd: the slot that holds the state flips between calls, and the grey must follow it
        for mode in modes:
            us = None
            if mode != "philox":
                us = torch.rand(Fn * k * step_n, B, 1, H, W, generator=gen).to(DEV)
                if mode == "bits":
                    us = ops.pack_fire_mask(us, 0.5, "dynca")
            out_dtype = torch.float32 if step_n == 4 else torch.uint8
            ops.persistent_steps = True
            want32, want8, want_h = _loop(ops, x, gray, cond, us, w, k, step_n, c_out, pad, seed, step0, two)
            want = want32 if out_dtype == torch.float32 else want8
            imgs, h = ops.dynca_clip_xc(x, gray, cond, us, w, k, step_n, c_out, pad, 0.5, seed, step0, two_scale=two, out_dtype=out_dtype)
            tag = (C, fc, c_cond, B, H, W, two, step_n, mode)
            assert imgs.shape == want.shape and imgs.dtype == out_dtype, tag
            for n in range(Fn * k):
                assert torch.equal(imgs[n], want[n]), (tag, "image", n)
            assert h.shape == (B, C, H, W) and torch.equal(h, want_h), (tag, "state")
            # the other route of the library gives the same bits (persistent launches <-> per-step launches)
            ops.persistent_steps = False
            imgs2, h2 = ops.dynca_clip_xc(x, gray, cond, us, w, k, step_n, c_out, pad, 0.5, seed, step0, two_scale=two, out_dtype=out_dtype)
            ops.persistent_steps = True
            assert torch.equal(imgs2, imgs) and torch.equal(h2, h), (tag, "persistent_steps off")
            # guard: without the grey before the repeats j > 0 the run is another one, so the comparison above sees the re-injection
            lazy32, lazy8, lazy_h = _loop(ops, x, gray, cond, us, w, k, step_n, c_out, pad, seed, step0, two, reinject=False)
            assert torch.equal(lazy32[0], want32[0]) and not torch.equal(lazy32[1:], want32[1:]) and not torch.equal(lazy_h, want_h), tag
            assert not torch.equal(lazy8[1:], want8[1:]), tag
    assert not torch.equal(want32[0], want32[-1])
    ops.check_errors()


# ------------------------------------------------------------------ 4. continuation and chunking
@pytest.mark.parametrize("mode", ["bits", "philox"])
@pytest.mark.parametrize("H,W", [(32, 48), (24, 40)])
def test_dynca_clip_xc_continues_across_calls(ops, mode, H, W):
    Fn, k, step_n, C, fc, seed, step0 = 4, 2, 3, 13, 96, 9, 100
    gen = torch.Generator().manual_seed(H + len(mode))
    gray = ops.clip_gray((torch.rand(Fn, 1, 3, H, W, generator=gen) * 2 - 1).to(DEV), "mean")
    cond = O.cpe2d(1, H, W).to(DEV)
    x = (torch.rand(1, C - 1, H, W, generator=gen) - 0.5).to(DEV)               # the reference's h: the driver adds the last channel
    w = ops.DyncaWeights(*_prm(C, fc, 2, 4), x)
    us = None
    if mode == "bits":
        us = ops.pack_fire_mask(torch.rand(Fn * k * step_n, 1, 1, H, W, generator=gen).to(DEV), 0.5, "dynca")
    whole, hw = ops.dynca_clip_xc(x, gray, cond, us, w, k, step_n, 3, "replicate", 0.5, seed, step0, two_scale=True)
    half = 2 * k * step_n
    a, ha = ops.dynca_clip_xc(x, gray[:2], cond, None if us is None else us[:half], w, k, step_n, 3, "replicate", 0.5, seed, step0, two_scale=True)
    assert ha.shape == (1, C, H, W)
    for cont in (ha, ha[:, :-1]):             # with or without the evolved extra channel: it is replaced before the next call
        b, hb = ops.dynca_clip_xc(cont, gray[2:], cond, None if us is None else us[half:], w, k, step_n, 3, "replicate", 0.5, seed, step0 + half,
                                  two_scale=True)
        assert torch.equal(torch.cat([a, b]), whole) and torch.equal(hb, hw)
    ops.check_errors()


def _model(scales=(0,), C=13, fc=96, seed=0, pos_emb="CPE"):
    from ncahip.models.dynca_extra import DyNCA
    torch.manual_seed(seed)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", pos_emb=pos_emb, perception_scales=list(scales), device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


@torch.no_grad()
def _hand_loop(m, frames, step_n, k, gray_fn=lambda f: f.mean(1, keepdim=True), state=None, out_dtype=torch.float32):
    """ExtraChannels/utils/misc/video_utils.py:66-82 over the module's forward_nsteps; frames [F,3,H,W] float32 on the device."""
    h = m.seed(1, size=(frames.shape[3], frames.shape[2])) if state is None else state
    imgs = []
    for f in range(frames.shape[0]):
        for _ in range(k):
            h = torch.cat((h, gray_fn(frames[f:f + 1]).to(h.dtype)), 1)
            state_, rgb = m.forward_nsteps(h, step_n)
            h = state_[:, :-1]
            img = rgb.float().clamp(-1.0, 1.0) * 0.5 + 0.5
            imgs.append((img * 255.0).to(torch.uint8).permute(0, 2, 3, 1) if out_dtype == torch.uint8 else img)
    return torch.cat(imgs), h


@pytest.mark.parametrize("rng", ["torch", "philox"])
@pytest.mark.parametrize("scales", [(0,), (0, 1)])
def test_stylize_clip_xc_does_not_depend_on_frames_per_call(ops, rng, scales):
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
        assert imgs.shape == (8, 32, 48, 3) and imgs.dtype == torch.uint8 and imgs.is_cuda and h.shape == (1, m.c_in - 1, 32, 48)
        res.append((imgs, h.clone(), torch.cuda.get_rng_state()))
    for imgs, h, st in res[1:]:
        assert torch.equal(imgs, res[0][0]) and torch.equal(h, res[0][1]) and torch.equal(st, res[0][2])
    assert not torch.equal(res[0][0][0], res[0][0][-1])
    # and the returned state continues the clip
    torch.manual_seed(7)
    m._mask_step = 40
    a, ha = video.stylize_clip(m, frames[:2], step_n=3, steps_per_frame=2, out_dtype=torch.uint8)
    b, hb = video.stylize_clip(m, frames[2:], step_n=3, steps_per_frame=2, out_dtype=torch.uint8, state=ha)
    assert torch.equal(torch.cat([a, b]), res[0][0]) and torch.equal(hb, res[0][1])
    ops.check_errors()


# ------------------------------------------------------------------ 5. stylize_clip against the reference's loop and float64
def test_stylize_clip_xc_against_the_hand_loop_and_float64(ops):
    from ncahip import video
    H, W, Fn, k, step_n = 32, 48, 3, 2, 4
    m = _model()
    assert m.mask_rng == "torch"
    gen = torch.Generator().manual_seed(2)
    frames = torch.rand(Fn, 3, H, W, generator=gen) * 2 - 1
    torch.manual_seed(5)
    old, old_state = _hand_loop(m, frames.to(DEV), step_n, k)
    old_state, old_rng = old_state.clone(), torch.cuda.get_rng_state()
    torch.manual_seed(5)
    new, new_state = video.stylize_clip(m, frames.to(DEV), step_n=step_n, steps_per_frame=k)
    assert video.stylize_clip.last_path == "clip" and new.shape == old.shape == (Fn * k, 3, H, W)
    assert new_state.shape == old_state.shape == (1, 12, H, W)
    assert torch.equal(torch.cuda.get_rng_state(), old_rng)                      # the generator ends where the loop leaves it
    # the same masks once more, for the float64 evaluation of the loop (the oracle's DyNCA step, read-only)
    torch.manual_seed(5)
    masks = [ops.unpack_fire_mask(ops.draw_fire_masks(1, H, W, step_n, 0.5, "dynca", DEV), 1, H, W).cpu().double() for _ in range(Fn * k)]
    assert torch.equal(torch.cuda.get_rng_state(), old_rng)
    prm = {n: p.detach().cpu().double() for n, p in m.state_dict().items() if n in ("w1.weight", "w1.bias", "w2.weight", "w2.bias")}
    pos = O.cpe2d(1, H, W, dtype=torch.float64)
    h, ref = torch.zeros(1, 12, H, W, dtype=torch.float64), []
    for n in range(Fn * k):
        grey = frames[n // k].double().mean(0, keepdim=True)[None]               # RGBToGrayscale in float64
        x = O.dynca_nsteps(torch.cat((h, grey), 1), pos, [mk * 0.5 for mk in masks[n]], prm, "circular", 0.5)    # floor(0.5 m + 0.5) = m
        ref.append((O.dynca_to_rgb(x, 3)[0].clamp(-1, 1) + 1) / 2)
        h = x[:, :-1]
    ref = torch.stack(ref)
    e_loop, e_clip = float((old.cpu().double() - ref).abs().max()), float((new.cpu().double() - ref).abs().max())
    diff = float((old.cpu().double() - new.cpu().double()).abs().max())
    sdiff = float((old_state - new_state).abs().max())
    print(f"stylize_clip (extra channel) vs float64: hand loop {e_loop:.3e}, clip route {e_clip:.3e}; loop vs clip {diff:.3e} "
          f"(final state {sdiff:.3e}); image std {float(ref.std()):.3e}")
    assert float(ref.std()) > 1e-3                                               # the images have content
    # two independent fp32 orderings of the same sums: the clip route may be at most twice as far from float64 as the hand loop
    assert e_clip <= 2 * e_loop + 1e-6, (e_loop, e_clip)
    assert diff <= e_loop + e_clip + 1e-12                                       # hence the two routes agree (triangle inequality)
    ops.check_errors()


# ------------------------------------------------------------------ 6. routes and errors
def test_other_scale_sets_and_bf16_states_take_the_loop(ops):
    from ncahip import video
    gen = torch.Generator().manual_seed(8)
    frames = (torch.rand(2, 3, 32, 48, generator=gen) * 2 - 1).to(DEV)
    u8 = ((frames * 0.5 + 0.5) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    m3 = _model(scales=(0, 1, 2))
    bf = lambda: torch.zeros(1, 12, 32, 48, device=DEV, dtype=torch.bfloat16)
    for m, state in ((m3, lambda: None), (_model(), bf)):
        for out_dtype, shape in ((torch.float32, (4, 3, 32, 48)), (torch.uint8, (4, 32, 48, 3))):
            torch.manual_seed(3)
            imgs, h = video.stylize_clip(m, frames, step_n=2, steps_per_frame=2, out_dtype=out_dtype, state=state())
            assert video.stylize_clip.last_path == "loop" and imgs.shape == shape and imgs.dtype == out_dtype and h.shape == (1, 12, 32, 48)
            torch.manual_seed(3)
            want, want_h = _hand_loop(m, frames, 2, 2, state=state(), out_dtype=out_dtype)
            assert torch.equal(imgs, want) and torch.equal(h, want_h), out_dtype
            assert float(imgs.float().std()) > 0
    # uint8 frames and the luma on the loop route: the widening and the grey of the edge family's loop
    torch.manual_seed(3)
    imgs, h = video.stylize_clip(m3, u8, step_n=2, gray="luma")
    torch.manual_seed(3)
    want, want_h = _hand_loop(m3, video._widen(u8), 2, 1, gray_fn=video.rgb_to_grayscale)
    assert video.stylize_clip.last_path == "loop" and torch.equal(imgs, want) and torch.equal(h, want_h)
    video.stylize_clip(_model(), frames, step_n=2)
    assert video.stylize_clip.last_path == "clip"
    video.stylize_clip(_model(pos_emb=None), frames, step_n=2)                   # no positional encoding: c_cond = 0
    assert video.stylize_clip.last_path == "clip"
    with pytest.raises(ValueError, match="c_in - 1"):
        video.stylize_clip(_model(), frames, state=torch.zeros(1, 13, 32, 48, device=DEV))
    ops.check_errors()


def test_sticky_error_word_refuses_the_xc_clip(ops):
    from ncahip._capi import NcaHipError
    gen = torch.Generator().manual_seed(6)
    x = (torch.rand(1, 13, 32, 48, generator=gen) - 0.5).to(DEV)
    gray = ops.clip_gray((torch.rand(2, 1, 3, 32, 48, generator=gen) * 2 - 1).to(DEV), "mean")
    cond = O.cpe2d(1, 32, 48).to(DEV)
    w = ops.DyncaWeights(*_prm(13, 96, 2, 1), x)
    ops.check_errors()
    assert ops.lib().ncahip_debug_inject_error(1) == 0
    try:
        for persist in (True, False):
            ops.persistent_steps = persist
            with pytest.raises(NcaHipError, match="device-side failure"):
                ops.dynca_clip_xc(x, gray, cond, None, w, 1, 4)
    finally:
        ops.persistent_steps = True
        ops.lib().ncahip_check_errors(ops._stream(), 1)      # never leave the word set for later tests
    ops.check_errors()
    imgs, _ = ops.dynca_clip_xc(x, gray, cond, None, w, 1, 4)
    assert bool(torch.isfinite(imgs).all())
