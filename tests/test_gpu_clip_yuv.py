"""GPU tests of planar YUV 4:2:0 clip frames (csrc/nca_yuv.hip, the planar loader of csrc/nca_resize.hip, ncahip.video's pixel_format
arguments) and of the overlapped upload of pinned frames.  The kernels are held against ops.yuv420_to_rgb_host (the contract in numpy,
itself held against float64 in tests/test_clip_yuv_host.py), the fused resize against conversion + resize and against Pillow, the clip
calls against the same calls on the mirror's RGB frames.  Every comparison is torch.equal."""
import numpy as np
import pytest
import torch

from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMATS = ("i420", "nv12")
MODES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
FILTERS = ("bicubic", "lanczos")


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        o.check_errors()                      # nothing recorded a device-side failure in this module


def planar_frames(N, h, w, fmt, seed):
    """Random planar frames [N, 3h/2, w] (host): frame 1, when there is one, saturated so that both clamps act."""
    gen = torch.Generator().manual_seed(seed)
    Y = torch.randint(0, 256, (N, h * w), generator=gen, dtype=torch.uint8)
    U = torch.randint(0, 256, (N, h // 2, w // 2), generator=gen, dtype=torch.uint8)
    V = torch.randint(0, 256, (N, h // 2, w // 2), generator=gen, dtype=torch.uint8)
    if N > 1:
        Y[1], U[1], V[1] = (Y[1] > 127).to(torch.uint8) * 255, (U[1] > 127).to(torch.uint8) * 255, (V[1] > 127).to(torch.uint8) * 255
    chroma = torch.cat((U.reshape(N, -1), V.reshape(N, -1)), 1) if fmt == "i420" else torch.stack((U, V), -1).reshape(N, -1)
    return torch.cat((Y, chroma), 1).reshape(N, 3 * h // 2, w).contiguous()


def off_by_one(frames):
    """The same frames on the device in a tensor that starts 1 byte into its storage."""
    buf = torch.empty(frames.numel() + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(frames.shape)
    view.copy_(frames)
    assert view.data_ptr() % 4 != 0 and view.is_contiguous()
    return view


# ------------------------------------------------------------------ 1. the conversion launch against the host mirror
@pytest.mark.parametrize("matrix,rng", MODES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_conversion_equals_the_host_mirror(ops, fmt, matrix, rng):
    from ncahip import video
    for h, w in [(2, 2), (2, 6), (6, 10), (4, 18), (70, 130)]:      # one chroma sample; plane starts at every byte phase; several blocks
        frames = planar_frames(3, h, w, fmt, 100 * h + w)
        want = ops.yuv420_to_rgb_host(frames, fmt, matrix, rng)
        dev = frames.to(DEV)
        for N in (1, 3):
            got = ops.yuv420_to_rgb(dev[:N], fmt, matrix, rng)
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (N, h, w, 3)
            assert torch.equal(got.cpu(), want[:N]), (h, w, N)
        assert torch.equal(video.yuv420_to_rgb(dev, fmt, matrix, rng).cpu(), want)
        assert torch.equal(ops.yuv420_to_rgb(off_by_one(frames), fmt, matrix, rng).cpu(), want), (h, w, "1 byte into the storage")
        for box in [(1, 1, 5, 3), (0, 0, w, h), (w - 1, h - 1, 1, 1), (1, 0, w - 1, h)]:
            if box[0] + box[2] > w or box[1] + box[3] > h:
                continue
            got = ops.yuv420_to_rgb(dev, fmt, matrix, rng, crop=box)          # crop_w * crop_h * 3 = 45: frames share output dwords
            assert torch.equal(got.cpu(), ops.yuv420_to_rgb_host(frames, fmt, matrix, rng, crop=box)), (h, w, box)
    ops.check_errors()


# ------------------------------------------------------------------ 2. the resize that converts in its loader
def _check_fused(ops, frames, fmt, mode, size, crop, filt):
    """resize_frames(pixel_format=...) on the device: equal to the conversion launch followed by the RGB resize, and to Pillow applied to
    the mirror's RGB."""
    from PIL import Image
    from ncahip import video
    h, w = frames.shape[1] // 3 * 2, frames.shape[2]
    dev = frames.to(DEV)
    got = video.resize_frames(dev, size, crop, filt, pixel_format=fmt, yuv_matrix=mode[0], yuv_range=mode[1])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (frames.shape[0],) + tuple(size) + (3,)
    two = video.resize_frames(video.yuv420_to_rgb(dev, fmt, *mode), size, crop, filt)
    assert torch.equal(got, two), (h, w, size, crop, filt, fmt)
    x0, y0, cw, ch = (0, 0, w, h) if crop is None else video.reference_crop(crop, h, w) if isinstance(crop, str) else crop
    pil_filter = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    rgb = ops.yuv420_to_rgb_host(frames.numpy(), fmt, *mode)
    want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(f[y0:y0 + ch, x0:x0 + cw])).resize((size[1], size[0]), pil_filter)) for f in rgb])
    assert np.array_equal(got.cpu().numpy(), want), (h, w, size, crop, filt, fmt)
    return got


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_resize_equals_conversion_then_resize(ops, fmt, filt):
    pytest.importorskip("PIL.Image")
    mode = ("bt709", "limited") if fmt == "i420" else ("bt601", "full")
    frames = planar_frames(2, 36, 64, fmt, 1)
    for crop in ("dynca", "conditioned", (3, 1, 31, 29), None):                # an odd origin and an odd size among them
        _check_fused(ops, frames, fmt, mode, (16, 16), crop, filt)
    # several column blocks, staged segments that begin on odd pixels
    wide = planar_frames(2, 40, 200, fmt, 2)
    _check_fused(ops, wide, fmt, mode, (8, 130), None, filt)
    _check_fused(ops, wide, fmt, mode, (8, 130), (1, 1, 197, 37), filt)
    # up-scaling, one frame, and a tensor 1 byte into its storage
    _check_fused(ops, planar_frames(1, 6, 10, fmt, 3), fmt, mode, (9, 21), None, filt)
    got = ops.clip_resize_yuv420(off_by_one(frames), (16, 16), (3, 1, 31, 29), filt, fmt, *mode)
    assert torch.equal(got, _check_fused(ops, frames, fmt, mode, (16, 16), (3, 1, 31, 29), filt))
    ops.check_errors()


# ------------------------------------------------------------------ 3. the clip entry points
def _dynca(conditioning="edges"):
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning=conditioning, edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _dynca_loop():
    return _dynca("pos_emb")


def _dynca_extra():
    from ncahip.models.dynca_extra import DyNCA
    torch.manual_seed(0)
    m = DyNCA(13, 3, fc_dim=96, padding_mode="circular", pos_emb="CPE", perception_scales=[0], device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _conditioned():
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(0)
    return ConditionedNCA(target_shape=(3, 16, 16)).to(DEV)


def _runner(make):
    """run(frames, **kw) -> (images, state) of the model's clip entry point from the same fire-mask position, and the entry point."""
    from ncahip import video
    m = make()
    m.mask_rng, m.mask_seed = "philox", 11
    fn = video.stylize_clip_conditioned if make is _conditioned else video.stylize_clip
    route = "loop" if make is _dynca_loop else "clip"

    def run(frames, mask_step=40, **kw):
        m._mask_step = mask_step
        imgs, h = fn(m, frames, step_n=2, out_dtype=torch.uint8, **kw)
        assert fn.last_path == route
        return imgs.clone(), h.clone()

    return run, fn


@pytest.mark.parametrize("sized", [False, True])
@pytest.mark.parametrize("make", [_dynca, _dynca_loop, _dynca_extra, _conditioned])
def test_clip_calls_equal_the_same_calls_on_the_mirrors_rgb(ops, make, sized):
    run, _ = _runner(make)
    kw = {"size": (16, 16)} if sized else {}
    h, w = (36, 64) if sized else (16, 16)
    for fmt, mode in (("i420", ("bt709", "limited")), ("nv12", ("bt601", "full"))):
        frames = planar_frames(5, h, w, fmt, 7)
        rgb = ops.yuv420_to_rgb_host(frames, fmt, *mode)
        want, want_h = run(rgb, **kw)
        assert tuple(want.shape) == (5, 16, 16, 3)
        for per_call in (1, 2, 32):
            for fr in (frames, frames.to(DEV)):
                got, got_h = run(fr, frames_per_call=per_call, pixel_format=fmt, yuv_matrix=mode[0], yuv_range=mode[1], **kw)
                assert torch.equal(got, want) and torch.equal(got_h, want_h), (fmt, per_call, fr.device)
    ops.check_errors()


# ------------------------------------------------------------------ 4. pinned frames: uploads on the side stream
@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_overlapped_upload_of_pinned_frames(ops, make):
    run, fn = _runner(make)
    rgb = torch.randint(0, 256, (5, 36, 64, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    for frames, kw in ((rgb, {}), (planar_frames(5, 36, 64, "i420", 9), {"pixel_format": "i420"})):
        kw = {"size": (16, 16), **kw}
        pinned = frames.pin_memory()
        assert pinned.is_pinned() and not frames.is_pinned()
        for per_call in (1, 2):
            want, want_h = run(frames.to(DEV), frames_per_call=per_call, **kw)
            assert fn.last_upload == "sync"
            plain, plain_h = run(frames, frames_per_call=per_call, **kw)
            assert fn.last_upload == "sync" and torch.equal(plain, want) and torch.equal(plain_h, want_h)
            got, got_h = run(pinned, frames_per_call=per_call, **kw)
            assert fn.last_upload == "overlapped" and torch.equal(got, want) and torch.equal(got_h, want_h), per_call
            # a second call continued from the returned state: two halves give the whole
            a, ha = run(pinned[:2], frames_per_call=per_call, **kw)
            b, hb = run(pinned[2:], mask_step=40 + 2 * 2, frames_per_call=per_call, state=ha, **kw)
            assert fn.last_upload == "overlapped" and torch.equal(torch.cat([a, b]), want) and torch.equal(hb, want_h), per_call
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_pinned_frames_on_a_stream_of_the_callers(ops, make):
    """The side stream's copies are ordered against the stream the call runs on, not the default stream."""
    run, fn = _runner(make)
    rgb = torch.randint(0, 256, (5, 36, 64, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    for frames, kw in ((rgb, {"size": (16, 16)}), (planar_frames(5, 36, 64, "i420", 9), {"size": (16, 16), "pixel_format": "i420"})):
        want, want_h = run(frames.to(DEV), frames_per_call=2, **kw)
        pinned = frames.pin_memory()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got, got_h = run(pinned, frames_per_call=2, **kw)
        assert fn.last_upload == "overlapped"
        s.synchronize()
        assert torch.equal(got, want) and torch.equal(got_h, want_h)
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_pinned_buffer_may_be_overwritten_when_the_call_returns(ops, make):
    """As with the blocking copies: when the clip call returns, no copy out of the caller's pinned buffer is in flight.  The compute
    stream is kept busy before each call (the side stream's copies queue behind it), the buffer is overwritten the moment the call
    returns -- a decoder writing the next clip into the same buffer -- and the results are those of the untouched frames."""
    run, fn = _runner(make)
    rgb = torch.randint(0, 256, (5, 36, 64, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    busy = torch.randn(2048, 2048, device=DEV)
    for frames, kw in ((rgb, {"size": (16, 16)}), (planar_frames(5, 36, 64, "i420", 9), {"size": (16, 16), "pixel_format": "i420"})):
        for per_call in (2, 32):                                               # several chunks; one chunk: the only copy is the last
            want, want_h = run(frames.to(DEV), frames_per_call=per_call, **kw)
            pinned = frames.pin_memory()
            for _ in range(40):
                busy @ busy
            got, got_h = run(pinned, frames_per_call=per_call, **kw)
            pinned.fill_(0)
            assert fn.last_upload == "overlapped"
            assert torch.equal(got, want) and torch.equal(got_h, want_h), per_call
    ops.check_errors()
