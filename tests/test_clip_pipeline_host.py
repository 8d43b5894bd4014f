"""Host-side checks of the chunk pipeline both clip calls run on (ncahip.video._run_clip) and of ops.ImageSpec, on CPU tensors (no GPU):
the loop routes of stylize_clip and stylize_clip_conditioned across frames_per_call, the image formats and out=; an exception from the
model in the middle of a clip; empty clips; the spec's table of shapes, dtypes and format words."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H, W, K, STEP_N = 5, 6, 10, 2, 2
ENTRIES = ("stylize_clip", "stylize_clip_conditioned")
IMAGES = [(torch.float32, "rgb24"), (torch.uint8, "rgb24"), (torch.uint8, "i420")]


@pytest.fixture(scope="module", autouse=True)
def _library():
    from ncahip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()


def _image_shape(dtype, fmt, h=H, w=W):
    return (3 * h // 2, w) if fmt != "rgb24" else ((h, w, 3) if dtype == torch.uint8 else (3, h, w))


class _HostModel:
    """The surface stylize_clip's loop route uses, in torch ops on the host (the DyNCA drop-in itself has no CPU path).  fail_at: the
    forward_nsteps call that raises."""
    device = torch.device("cpu")
    conditioning = "edges"
    perception_scales = [0]
    c_in, c_out = 6, 3

    def __init__(self, fail_at=None):
        self.calls, self.fail_at = 0, fail_at

    def seed(self, n, size=128):
        sx, sy = (size, size) if isinstance(size, int) else size
        return torch.zeros(n, self.c_in, sy, sx)

    def forward_nsteps(self, h, step_n, cond_img=None):
        self.calls += 1
        if self.calls == self.fail_at:
            raise RuntimeError("boom")
        h = h + 0.05 * step_n * (cond_img + 0.5)
        return h, h[:, :self.c_out] * 2.0 + torch.linspace(-1.5, 1.5, h.shape[-1])


def _host_cond(fail_at=None):
    """A tiny ConditionedNCA on the CPU (C = 3 + 1 + 4) whose grow is torch ops on the host; fail_at: the grow call that raises."""
    from ncahip.nca import ConditionedNCA

    class HostCond(ConditionedNCA):
        calls = 0

        def grow(self, x, num_steps, goal):
            self.calls += 1
            if self.calls == fail_at:
                raise RuntimeError("boom")
            return x + 0.04 * num_steps * (goal.mean(1, keepdim=True) - 0.2) + torch.linspace(-0.05, 0.05, x.shape[-1])

    return HostCond(target_shape=(3, H, H), num_hidden_channels=4)


def _frames():
    return torch.randint(0, 256, (F, H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)


def _call(entry, frames, fail_at=None, **kw):
    """(images, state, the entry point) of one call on a fresh model."""
    from ncahip import video
    kw = dict(step_n=STEP_N, steps_per_frame=K, **kw)
    if entry == "stylize_clip":
        fn, res = video.stylize_clip, video.stylize_clip(_HostModel(fail_at), frames, **kw)
    else:
        if frames.shape[1] != frames.shape[2]:          # state=None seeds a square grid only
            kw["state"] = torch.zeros(1, 8, *frames.shape[1:3])
        fn, res = video.stylize_clip_conditioned, video.stylize_clip_conditioned(_host_cond(fail_at), frames, **kw)
    return res[0], res[1], fn


_REFERENCE = {}


def _reference(entry, dtype, fmt):
    """frames_per_call = F, out=None: computed once per (entry, image format) and left unchanged."""
    key = (entry, dtype, fmt)
    if key not in _REFERENCE:
        _REFERENCE[key] = _call(entry, _frames(), out_dtype=dtype, out_format=fmt, frames_per_call=F)[:2]
    return _REFERENCE[key]


@pytest.mark.parametrize("dtype,fmt", IMAGES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_loop_route_across_chunking_formats_and_out(entry, dtype, fmt):
    from ncahip import video
    want, want_state = _reference(entry, dtype, fmt)
    assert want.shape == (F * K,) + _image_shape(dtype, fmt) and want.dtype == dtype
    assert want_state.shape == ((1, 6, H, W) if entry == "stylize_clip" else (1, 8, H, W))
    assert len({bytes(img.numpy().tobytes()) for img in want}) == F * K         # every (frame, k) moved the image
    if fmt != "rgb24":
        assert torch.equal(want, video.rgb_to_yuv420(_reference(entry, torch.uint8, "rgb24")[0], fmt))
    for per_call in (1, 2, F):                                                   # 2: a ragged last chunk
        for with_out in (False, True):
            out = torch.full((F * K,) + _image_shape(dtype, fmt), 7, dtype=dtype) if with_out else None
            assert out is None or not out.is_pinned()
            images, state, fn = _call(entry, _frames(), out_dtype=dtype, out_format=fmt, frames_per_call=per_call, out=out)
            assert torch.equal(images, want) and torch.equal(state, want_state), (per_call, with_out)
            assert torch.equal(fn.last_state, want_state)
            assert (images is out and fn.last_download == "sync") if with_out else fn.last_download is None
            assert fn.last_upload == "sync" and fn.last_path == "loop"


@pytest.mark.parametrize("with_out", [False, True])
@pytest.mark.parametrize("entry", ENTRIES)
def test_an_exception_from_the_model_in_the_second_chunk(entry, with_out):
    """frames_per_call = 1: the fourth model call is the second step of the second chunk."""
    want, want_state = _reference(entry, torch.uint8, "rgb24")
    out = torch.full((F * K, H, W, 3), 7, dtype=torch.uint8) if with_out else None
    with pytest.raises(RuntimeError) as caught:
        _call(entry, _frames(), fail_at=4, out_dtype=torch.uint8, frames_per_call=1, out=out)
    assert type(caught.value) is RuntimeError and caught.value.args == ("boom",)
    if with_out:          # the first chunk had been delivered, nothing after it
        assert torch.equal(out[:K], want[:K]) and bool((out[K:] == 7).all())
    # nothing is left attached or half-open: the same call on a fresh model gives what it gave before
    out = torch.empty(F * K, H, W, 3, dtype=torch.uint8) if with_out else None
    images, state, fn = _call(entry, _frames(), out_dtype=torch.uint8, frames_per_call=1, out=out)
    assert torch.equal(images, want) and torch.equal(state, want_state) and (images is out or not with_out)
    assert fn.last_download == ("sync" if with_out else None)


@pytest.mark.parametrize("dtype,fmt", IMAGES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_empty_clips(entry, dtype, fmt):
    w = W if entry == "stylize_clip" else H                 # the conditioned call seeds a square grid
    images, state, fn = _call(entry, _frames()[:0, :, :w], out_dtype=dtype, out_format=fmt)
    assert images.shape == (0,) + _image_shape(dtype, fmt, H, w) and images.dtype == dtype
    assert state.shape == ((1, 6, H, W) if entry == "stylize_clip" else (1, 8, H, H))       # the seed's
    assert fn.last_state is state and fn.last_path == "loop" and fn.last_download is None


def test_image_spec_table():
    from ncahip import _capi, ops
    f32, u8 = torch.float32, torch.uint8
    #        arguments after (c_out, H, W) are appended                   shape          dtype  planar  format word
    table = [((f32, "rgb24", "bt709", "limited", 1),                     (1, 6, 10),    f32,   False,  _capi.CLIP_F32_NCHW),
             ((f32, "rgb24", "bt709", "limited", 3),                     (3, 6, 10),    f32,   False,  _capi.CLIP_F32_NCHW),
             ((u8, "rgb24", "bt709", "limited", 1),                      (6, 10, 1),    u8,    False,  _capi.CLIP_U8_NHWC),
             ((u8, "rgb24", "bt601", "full", 3),                         (6, 10, 3),    u8,    False,  _capi.CLIP_U8_NHWC),
             ((u8, "i420", "bt709", "limited", 3),                       (9, 10),       u8,    True,   _capi.clip_yuv420(0, 1, 0)),
             ((u8, "i420", "bt601", "full", 3),                          (9, 10),       u8,    True,   _capi.clip_yuv420(0, 0, 1)),
             ((u8, "nv12", "bt709", "full", 3),                          (9, 10),       u8,    True,   _capi.clip_yuv420(1, 1, 1)),
             ((u8, "nv12", "bt601", "limited", 3),                       (9, 10),       u8,    True,   _capi.clip_yuv420(1, 0, 0))]
    assert (_capi.CLIP_F32_NCHW, _capi.CLIP_U8_NHWC, _capi.clip_yuv420(1, 0, 0), _capi.clip_yuv420(1, 1, 1)) == (0, 1, 0x101, 0x107)
    for args, shape, dtype, planar, word in table:
        spec = ops.ImageSpec.of(*args, 6, 10)
        assert (spec.shape, spec.out_dtype, spec.planar, spec.fmt) == (shape, dtype, planar, word), args
        assert ops._clip_img_fmt(*args, 6, 10) == word
        imgs = spec.images(4, 2, "cpu")
        assert imgs.shape == (4, 2) + shape and imgs.dtype == dtype, args
        assert spec.keywords == {"out_dtype": args[0], "out_format": args[1], "yuv_matrix": args[2], "yuv_range": args[3]}
        with pytest.raises(ValueError, match="images must be a contiguous"):
            spec.images(4, 2, "cpu", into=imgs)                                # a driver writes into device memory only
        with pytest.raises(AttributeError):
            spec.H = 8                                                         # immutable
    assert ops.ImageSpec.of(u8) == ops.ImageSpec.of(u8, "rgb24", "bt709", "limited", 3, 2, 2) == (u8, "rgb24", "bt709", "limited", 3, 2, 2, 1, (2, 2, 3), False)
    # the refusals, before anything runs
    with pytest.raises(ValueError, match="needs out_dtype=torch.uint8"):
        ops.ImageSpec.of(f32, "i420", "bt709", "limited", 3, 6, 10)
    with pytest.raises(ValueError, match="c_out == 3"):
        ops.ImageSpec.of(u8, "i420", "bt709", "limited", 1, 6, 10)
    with pytest.raises(ValueError, match="even H and W"):
        ops.ImageSpec.of(u8, "nv12", "bt709", "limited", 3, 7, 10)
    with pytest.raises(ValueError, match="even H and W"):
        ops.ImageSpec.of(u8, "nv12", "bt709", "limited", 3, 6, 9)
    with pytest.raises(ValueError, match="out_format must be one of"):
        ops.ImageSpec.of(u8, "yuv444", "bt709", "limited", 3, 6, 10)
    with pytest.raises(ValueError, match="yuv_matrix"):
        ops.ImageSpec.of(u8, "i420", "bt2020", "limited", 3, 6, 10)
    with pytest.raises(TypeError, match="float32 .* or uint8"):
        ops.ImageSpec.of(torch.float16, "rgb24", "bt709", "limited", 3, 6, 10)
    assert ops.ImageSpec.of(u8, "rgb24", "bt2020", "tv", 3, 7, 9).fmt == 1        # rgb24 looks at neither the matrix nor the parity, as before


def test_frames_dims():
    from ncahip import ops
    assert ops._frames_dims(torch.zeros(2, 1, 3, 4, 5)) == (0, 2, 1, 3, 4, 5)
    assert ops._frames_dims(torch.zeros(2, 1, 4, 5, 3, dtype=torch.uint8)) == (1, 2, 1, 3, 4, 5)
    with pytest.raises(TypeError):
        ops._frames_dims(torch.zeros(2, 1, 3, 4, 5, dtype=torch.float64))
    for bad in (torch.zeros(2, 3, 4, 5), torch.zeros(2, 4, 5, 3, dtype=torch.uint8), torch.zeros(2, 1, 1, 4, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops._frames_dims(bad)
