"""GPU tests of planar YUV 4:2:0 images out of the clip calls (csrc/nca_yuv_out.hip, the planar emit of csrc/nca_clip.hip, ncahip.video's
out_format= and out= arguments).  The conversion launch is held against ops.rgb_to_yuv420_host (the contract in numpy, itself held against
float64 in tests/test_clip_yuv_out_host.py), the fused emits against the uint8 emit followed by the conversion launch, the clip calls
against the same calls with RGB uint8 output passed through the mirror, and out= against the call without it.  Every comparison is
torch.equal."""
import ctypes

import pytest
import torch

from gpu_ops import gpu_ops
from test_gpu_clip_yuv import _conditioned, _dynca, _dynca_extra, _dynca_loop, planar_frames

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = ("i420", "nv12")
MODES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
SIZES = [(2, 2), (2, 6), (6, 10), (6, 34), (18, 66)]      # one half lane; W % 4 == 2: rows and planes at every phase; more than one workgroup
GUARD, FILL = 16, 0xA5


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        o.check_errors()                      # nothing recorded a device-side failure in this module


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def guarded(nbytes, off):
    """(buffer, view): `nbytes` bytes that start GUARD + off bytes into a 256-byte aligned buffer pre-filled with FILL."""
    buf = torch.full((GUARD + 3 + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0
    return buf, buf[GUARD + off:GUARD + off + nbytes]


def guards_intact(buf, off, nbytes):
    return bool((buf[:GUARD + off] == FILL).all()) and bool((buf[GUARD + off + nbytes:] == FILL).all())


def shifted(t, off):
    """The same tensor on the device, `off` bytes into an aligned storage."""
    buf = torch.empty(t.numel() * t.element_size() + 4, dtype=torch.uint8, device=DEV)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 4 == off
    return view


def layout_word(ops, fmt, mode):
    from ncahip import _capi
    return _capi.clip_yuv420(_capi.YUV_LAYOUTS[fmt], _capi.YUV_MATRICES[mode[0]], _capi.YUV_RANGES[mode[1]])


# ------------------------------------------------------------------ 1. the conversion launch against the host mirror
@pytest.mark.parametrize("matrix,rng", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_conversion_equals_the_host_mirror(ops, fmt, matrix, rng):
    from ncahip import _capi, video
    L, k = ops.lib(), ops.rgb_yuv_coeffs(matrix, rng)
    for h, w in SIZES:
        rgb = torch.randint(0, 256, (2, h, w, 3), generator=torch.Generator().manual_seed(100 * h + w), dtype=torch.uint8)
        rgb[1] = (rgb[1] > 127).to(torch.uint8) * 255                             # saturated colours: the limited range's ends
        want = ops.rgb_to_yuv420_host(rgb, fmt, matrix, rng).to(DEV)
        assert tuple(want.shape) == (2, 3 * h // 2, w)
        got = video.rgb_to_yuv420(rgb.to(DEV), fmt, matrix, rng)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want), (h, w)
        for N in (1, 2):
            nbytes = N * 3 * h * w // 2
            for soff in range(4):
                src = shifted(rgb[:N], soff)
                for doff in range(4):
                    buf, dst = guarded(nbytes, doff)
                    rc = L.ncahip_clip_rgb_to_yuv420_u8(P(src), _capi.YUV_LAYOUTS[fmt], N, h, w, k.ctypes.data, P(dst), ops._stream())
                    assert rc == 0, L.ncahip_last_error()
                    assert torch.equal(dst.view(N, 3 * h // 2, w), want[:N]), (h, w, N, soff, doff)
                    assert guards_intact(buf, doff, nbytes), (h, w, N, soff, doff)
    ops.check_errors()


# ------------------------------------------------------------------ 2. the fused emits against emit-uint8 followed by the conversion
def crafted_state(B, C, H, W, unit, seed):
    """A state whose image covers both sides of the clamp, exact 0 and 1, and values where img * 255 is an integer (no NaN: the uint8 of NaN
    is not part of the contract)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, H, W, generator=gen) * 3.0 - 1.0                         # below, inside and above either clamp range
    ints = torch.randint(0, 256, (B, C, H, W), generator=gen).float() / 255.0      # img * 255 an integer (up to the rounding of the division)
    ints = ints if unit else ints - 0.5                                            # DyNCA families: img = (clamp(2x, -1, 1) + 1) / 2
    pick = torch.rand(B, C, H, W, generator=gen)
    x = torch.where(pick < 0.3, ints, x)
    specials = torch.tensor([0.0, 1.0, -0.0, 0.5, -0.5, 1.0 / 255.0, 254.0 / 255.0, 0.999999, 1.000001, -1e-7, 2.0, -3.0, 127.5 / 255.0])
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=gen)[:min(flat.numel(), 4 * len(specials))]
    flat[idx] = specials.repeat(4)[:idx.numel()]
    return x.to(DEV)


@pytest.mark.parametrize("entry", ["emit", "emit_inject", "emit_unit"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_emit_equals_emit_then_conversion(ops, fmt, entry):
    L = ops.lib()
    C = {"emit": 12, "emit_inject": 4, "emit_unit": 20}[entry]
    unit = entry == "emit_unit"
    for mode in MODES:
        word = layout_word(ops, fmt, mode)
        for h, w in SIZES:
            for B in (1, 2):
                x = crafted_state(B, C, h, w, unit, 1000 * h + 10 * w + B)
                gray = torch.randn(B, h, w, generator=torch.Generator().manual_seed(h + w)).to(DEV)
                # the two launches: the uint8 image (and the inject), then the conversion
                x2 = x.clone()
                if entry == "emit":
                    rgb = ops.clip_emit(x2, 3, torch.uint8)
                elif entry == "emit_unit":
                    rgb = ops.clip_emit_unit(x2, torch.uint8)
                else:
                    rgb = ops.clip_emit_inject(x2, 3, gray, torch.uint8)
                    assert torch.equal(x2[:, C - 1], gray) and torch.equal(x2[:, :C - 1], x[:, :C - 1])
                want = ops.rgb_to_yuv420(rgb, fmt, *mode)
                assert torch.equal(want.cpu(), ops.rgb_to_yuv420_host(rgb.cpu(), fmt, *mode))
                # the Python entry point, then the C entry point at every byte offset of the image
                x1 = x.clone()
                kw = dict(out_format=fmt, yuv_matrix=mode[0], yuv_range=mode[1])
                got = (ops.clip_emit(x1, 3, torch.uint8, **kw) if entry == "emit" else ops.clip_emit_unit(x1, torch.uint8, **kw) if unit
                       else ops.clip_emit_inject(x1, 3, gray, torch.uint8, **kw))
                assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 3 * h // 2, w) and torch.equal(got, want), (mode, h, w, B)
                assert torch.equal(x1, x2), "the injected plane / the untouched channels differ from the separate launch's"
                nbytes = B * 3 * h * w // 2
                for doff in range(4):
                    buf, dst = guarded(nbytes, doff)
                    x1 = x.clone()
                    if entry == "emit":
                        rc = L.ncahip_clip_emit(P(x1), P(dst), word, B, C, 3, h, w, ops._stream())
                    elif unit:
                        rc = L.ncahip_clip_emit_unit(P(x1), P(dst), word, B, C, h, w, ops._stream())
                    else:
                        rc = L.ncahip_clip_emit_inject(P(x1), P(dst), word, P(gray), B, C, 3, h, w, ops._stream())
                    assert rc == 0, L.ncahip_last_error()
                    assert torch.equal(dst.view(B, 3 * h // 2, w), want), (mode, h, w, B, doff)
                    assert guards_intact(buf, doff, nbytes) and torch.equal(x1, x2), (mode, h, w, B, doff)
    ops.check_errors()


# ------------------------------------------------------------------ 3. the clip calls
def runner(make, step_n=2):
    """run(frames, **kw) -> (images, state, _mask_step after) of the model's clip entry point from the same fire-mask position."""
    from ncahip import video
    m = make()
    m.mask_rng, m.mask_seed = "philox", 11
    fn = video.stylize_clip_conditioned if make is _conditioned else video.stylize_clip
    route = "loop" if make is _dynca_loop else "clip"

    def run(frames, mask_step=40, **kw):
        m._mask_step = mask_step
        imgs, h = fn(m, frames, step_n=step_n, out_dtype=torch.uint8, **kw)
        assert fn.last_path == route
        return imgs, h.clone(), m._mask_step

    return run, fn, m


def rgb_frames(F, h, w, seed):
    return torch.randint(0, 256, (F, h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("make", [_dynca, _dynca_loop, _dynca_extra, _conditioned])
def test_clip_calls_equal_the_mirror_of_their_rgb_images(ops, make):
    run, fn, _ = runner(make)
    frames = rgb_frames(5, 16, 16, 7).to(DEV)
    rgb, want_h, want_step = run(frames)
    assert tuple(rgb.shape) == (5, 16, 16, 3) and fn.last_download is None
    for fmt, mode in (("i420", ("bt709", "limited")), ("nv12", ("bt601", "full"))):
        want = ops.rgb_to_yuv420_host(rgb.cpu(), fmt, *mode)
        for per_call in (1, 2, 5):
            got, h, step = run(frames, frames_per_call=per_call, out_format=fmt, out_yuv_matrix=mode[0], out_yuv_range=mode[1])
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (5, 24, 16)
            assert torch.equal(got.cpu(), want) and torch.equal(h, want_h) and step == want_step, (fmt, per_call)
            assert fn.last_download is None
    ops.check_errors()


def test_clip_call_with_bf16_precision_and_a_32_grid(ops):
    run, _, _ = runner(_dynca)
    frames = rgb_frames(5, 32, 32, 8).to(DEV)
    rgb, want_h, want_step = run(frames, precision="bf16", steps_per_frame=2)
    assert tuple(rgb.shape) == (10, 32, 32, 3)
    got, h, step = run(frames, precision="bf16", steps_per_frame=2, frames_per_call=2, out_format="nv12")
    assert torch.equal(got.cpu(), ops.rgb_to_yuv420_host(rgb.cpu(), "nv12", "bt709", "limited")) and torch.equal(h, want_h) and step == want_step
    assert ops.set_dynca_precision("f32") == "f32"                                # the mode is what it was
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_clip_call_planar_in_and_planar_out(ops, make):
    """Decoder-sized I420 frames in, NV12 images out, every existing option along: size, crop, pixel_format."""
    run, _, _ = runner(make)
    frames = planar_frames(5, 36, 64, "i420", 9)
    kw = dict(size=(16, 16), pixel_format="i420", yuv_matrix="bt601", yuv_range="full")
    rgb, want_h, want_step = run(frames, **kw)
    got, h, step = run(frames.pin_memory(), frames_per_call=2, out_format="nv12", out_yuv_matrix="bt601", out_yuv_range="limited", **kw)
    assert torch.equal(got.cpu(), ops.rgb_to_yuv420_host(rgb.cpu(), "nv12", "bt601", "limited")) and torch.equal(h, want_h) and step == want_step
    ops.check_errors()


# ------------------------------------------------------------------ 4. out=: delivery into a caller's tensor
@pytest.mark.parametrize("make", [_dynca, _dynca_loop, _conditioned])
def test_pinned_out_is_filled_on_the_side_stream(ops, make):
    run, fn, _ = runner(make)
    frames = rgb_frames(5, 16, 16, 3).to(DEV)
    for kw, shape in ((dict(out_format="i420"), (5, 24, 16)), ({}, (5, 16, 16, 3))):
        want, want_h, want_step = run(frames, **kw)
        want = want.cpu()
        for per_call in (1, 2, 3):
            out = torch.full(shape, FILL, dtype=torch.uint8).pin_memory()
            got, h, step = run(frames, frames_per_call=per_call, out=out, **kw)
            assert got is out and fn.last_download == "overlapped"
            assert torch.equal(out, want) and torch.equal(h, want_h) and step == want_step, (kw, per_call)
        # two consecutive calls continue the state into the two halves of one buffer
        out = torch.full(shape, FILL, dtype=torch.uint8).pin_memory()
        _, ha, _ = run(frames[:2], frames_per_call=1, out=out[:2], **kw)
        _, hb, step = run(frames[2:], mask_step=40 + 2 * 2, frames_per_call=2, state=ha, out=out[2:], **kw)
        assert fn.last_download == "overlapped" and torch.equal(out, want) and torch.equal(hb, want_h) and step == want_step
        # pageable and device tensors: a plain copy per chunk, the same bytes
        for out in (torch.full(shape, FILL, dtype=torch.uint8), torch.full(shape, FILL, dtype=torch.uint8, device=DEV)):
            got, h, _ = run(frames, frames_per_call=2, out=out, **kw)
            assert got is out and fn.last_download == "sync" and torch.equal(out.cpu(), want) and torch.equal(h, want_h)
        run(frames, **kw)
        assert fn.last_download is None
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_pinned_out_on_a_stream_of_the_callers(ops, make):
    """The side stream's copies are ordered against the stream the call runs on, not the default stream."""
    run, fn, _ = runner(make)
    frames = rgb_frames(5, 16, 16, 4).to(DEV)
    want, want_h, _ = run(frames, out_format="nv12")
    want = want.cpu()
    out = torch.full((5, 24, 16), FILL, dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, h, _ = run(frames, frames_per_call=2, out_format="nv12", out=out)
    assert got is out and fn.last_download == "overlapped" and torch.equal(out, want)      # valid at return: no synchronize before this line
    s.synchronize()
    assert torch.equal(h, want_h)
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_every_byte_of_a_pinned_out_is_valid_when_the_call_returns(ops, make):
    """The compute stream is kept busy before the call (the side stream's copies queue behind it); `out`, pre-filled with a sentinel, is read
    the moment the call returns, with no synchronize call in between: no sentinel is left where the image has another value."""
    run, fn, _ = runner(make)
    frames = rgb_frames(5, 16, 16, 5).to(DEV)
    busy = torch.randn(2048, 2048, device=DEV)
    for kw, shape in ((dict(out_format="i420"), (5, 24, 16)), ({}, (5, 16, 16, 3))):
        want = run(frames, **kw)[0].cpu()
        for per_call in (2, 32):                                                   # several chunks; one chunk: the only copy is the last
            out = torch.full(shape, FILL, dtype=torch.uint8).pin_memory()
            for _ in range(40):
                busy @ busy
            run(frames, frames_per_call=per_call, out=out, **kw)
            left = int(((out == FILL) & (want != FILL)).sum())
            assert fn.last_download == "overlapped" and left == 0 and torch.equal(out, want), (kw, per_call, left)
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_a_wrong_out_is_refused_before_any_work(ops, make):
    run, fn, m = runner(make)
    frames = rgb_frames(3, 16, 16, 6).to(DEV)
    gen_state = torch.cuda.get_rng_state()
    for bad in (torch.empty(3, 16, 16, 3, dtype=torch.uint8).pin_memory(), torch.empty(2, 24, 16, dtype=torch.uint8).pin_memory(),
                torch.empty(3, 24, 16, dtype=torch.float32, device=DEV), torch.empty(3, 24, 32, dtype=torch.uint8, device=DEV)[:, :, ::2]):
        m._mask_step = 40
        with pytest.raises(ValueError, match="out must be"):
            fn(m, frames, step_n=2, out_dtype=torch.uint8, out_format="i420", out=bad)
        assert m._mask_step == 40 and torch.equal(torch.cuda.get_rng_state(), gen_state)
    ops.check_errors()
