"""Host-side checks of planar YUV 4:2:0 clip frames (no GPU): the coefficients of ncahip_yuv_coeffs, ops.yuv420_to_rgb_host -- the integer
contract of include/ncahip.h in numpy -- against an independent float64 evaluation of the real-valued definition, the two layouts, crops,
the refusals of the Python and C entry points, and the CPU route of resize_frames(pixel_format=...) against Pillow."""
import ctypes

import numpy as np
import pytest
import torch

FORMATS = ("i420", "nv12")
MODES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
COEFFS = {("bt601", "limited"): (76309, 104597, -25675, -53279, 132201, 16), ("bt601", "full"): (65536, 91881, -22553, -46802, 116130, 0),
          ("bt709", "limited"): (76309, 117489, -13975, -34925, 138438, 16), ("bt709", "full"): (65536, 103206, -12276, -30679, 121609, 0)}


@pytest.fixture(scope="module")
def ops():
    from ncahip import ops as _ops
    return _ops


def planes(rng, N, h, w):
    return (rng.integers(0, 256, (N, h, w), dtype=np.uint8), rng.integers(0, 256, (N, h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (N, h // 2, w // 2), dtype=np.uint8))


def pack(Y, U, V, fmt):
    """[N, 3h/2, w] frames of the planes in one of the two layouts."""
    N, h, w = Y.shape
    chroma = np.concatenate((U.reshape(N, -1), V.reshape(N, -1)), axis=1) if fmt == "i420" else np.stack((U, V), axis=-1).reshape(N, -1)
    return np.concatenate((Y.reshape(N, -1), chroma), axis=1).reshape(N, 3 * h // 2, w)


def test_coefficients(ops):
    from ncahip import _capi
    L = ops.lib()
    for (matrix, rng), want in COEFFS.items():
        k = (ctypes.c_int32 * 6)()
        assert L.ncahip_yuv_coeffs(_capi.YUV_MATRICES[matrix], _capi.YUV_RANGES[rng], k) == 0
        assert tuple(k) == want, (matrix, rng)
        got = ops.yuv_coeffs(matrix, rng)
        assert got.dtype == np.int32 and tuple(int(v) for v in got) == want and ops.yuv_coeffs(matrix, rng) is got      # cached
    k = (ctypes.c_int32 * 6)()
    for matrix, rng in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        assert L.ncahip_yuv_coeffs(matrix, rng, k) == _capi.EINVAL
    assert L.ncahip_yuv_coeffs(0, 0, None) == _capi.EINVAL


def real_valued(Y, U, V, matrix, rng):
    """The real-valued definition in float64, rounded half up and clamped: [..., 3]."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    sy, sc, off = (255.0 / 219.0, 255.0 / 224.0, 16.0) if rng == "limited" else (1.0, 1.0, 0.0)
    y, u, v = sy * (Y.astype(np.float64) - off), sc * (U.astype(np.float64) - 128.0), sc * (V.astype(np.float64) - 128.0)
    rgb = np.stack((y + 2.0 * (1.0 - kr) * v, y - (2.0 * kb * (1.0 - kb) / kg) * u - (2.0 * kr * (1.0 - kr) / kg) * v, y + 2.0 * (1.0 - kb) * u), axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0.0, 255.0).astype(np.int64)


@pytest.mark.parametrize("matrix,rng", MODES)
def test_mirror_against_float64(ops, matrix, rng):
    """All 256^2 (U, V) pairs x 32 luma values (the ends of both ranges and their neighbours among them): the integer formula is never
    more than 1 away from the real-valued definition and differs from it on at most 1e-3 of any channel's values (over all 2^24
    triples: at most 5.2e-4)."""
    lumas = sorted({0, 15, 16, 17, 234, 235, 236, 255} | set(range(3, 255, 9)))
    assert len(lumas) >= 32
    # one frame per luma value: 512 x 512 pixels, every 2 x 2 block one (U, V) pair
    n = len(lumas)
    Y = np.repeat(np.array(lumas, dtype=np.uint8), 512 * 512).reshape(n, 512, 512)
    U = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (n, 256, 256))
    V = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (n, 256, 256))
    got = ops.yuv420_to_rgb_host(pack(Y, U, V, "i420"), "i420", matrix, rng)[:, ::2, ::2].astype(np.int64)      # one pixel per pair
    want = real_valued(Y[:, ::2, ::2], U, V, matrix, rng)
    diff = np.abs(got - want)
    frac = [float((diff[..., c] != 0).mean()) for c in range(3)]
    print(f"{matrix} {rng}: max |diff| {int(diff.max())}, differing fraction per channel {frac}")
    assert int(diff.max()) <= 1
    assert max(frac) <= 1e-3, frac
    assert int(got.min()) == 0 and int(got.max()) == 255                      # both clamps act


@pytest.mark.parametrize("matrix,rng", MODES)
def test_layouts_and_crops(ops, matrix, rng):
    gen = np.random.default_rng(3)
    for h, w in [(2, 2), (6, 10), (4, 18), (70, 130)]:
        Y, U, V = planes(gen, 2, h, w)
        a = ops.yuv420_to_rgb_host(pack(Y, U, V, "i420"), "i420", matrix, rng)
        b = ops.yuv420_to_rgb_host(pack(Y, U, V, "nv12"), "nv12", matrix, rng)
        assert a.dtype == np.uint8 and a.shape == (2, h, w, 3) and np.array_equal(a, b)
        # nearest chroma: the four pixels of a 2 x 2 block share (U, V) -- equal luma gives equal pixels
        flat = ops.yuv420_to_rgb_host(pack(np.full_like(Y, 120), U, V, "i420"), "i420", matrix, rng)
        assert np.array_equal(flat[:, 0::2, 0::2], flat[:, 1::2, 1::2]) and np.array_equal(flat[:, 0::2, 1::2], flat[:, 1::2, 0::2])
        for box in [(1, 1, 5, 3), (0, 0, w, h), (1, 0, w - 1, h), (w - 1, h - 1, 1, 1), (3, 1, 7, 3)]:
            x0, y0, cw, ch = box
            if x0 + cw > w or y0 + ch > h:
                continue
            for fmt in FORMATS:
                got = ops.yuv420_to_rgb_host(pack(Y, U, V, fmt), fmt, matrix, rng, crop=box)
                assert np.array_equal(got, a[:, y0:y0 + ch, x0:x0 + cw]), (h, w, box, fmt)
    # tensors in, tensors out; video.yuv420_to_rgb runs the mirror for CPU frames
    from ncahip import video
    t = torch.from_numpy(pack(Y, U, V, "nv12"))
    got = video.yuv420_to_rgb(t, "nv12", matrix, rng)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and np.array_equal(got.numpy(), a)


def test_python_refusals(ops):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    from ncahip.nca import ConditionedNCA
    m = DyNCA(12, 3, fc_dim=96, conditioning="edges", device=torch.device("cpu"))
    nca = ConditionedNCA(target_shape=(3, 4, 4), num_hidden_channels=4)
    good = torch.zeros(2, 12, 10, dtype=torch.uint8)                         # two 8 x 10 frames
    calls = {
        "yuv420_to_rgb": lambda fr, **kw: video.yuv420_to_rgb(fr, kw.pop("pixel_format", "i420"), **kw),
        "resize_frames": lambda fr, **kw: video.resize_frames(fr, (4, 4), None, "bicubic", **{"pixel_format": "i420", **kw}),
        "stylize_clip": lambda fr, **kw: video.stylize_clip(m, fr, step_n=1, **{"pixel_format": "i420", **kw}),
        "stylize_clip size": lambda fr, **kw: video.stylize_clip(m, fr, step_n=1, size=(4, 4), **{"pixel_format": "i420", **kw}),
        "stylize_clip_conditioned": lambda fr, **kw: video.stylize_clip_conditioned(nca, fr, step_n=1, size=(4, 4), **{"pixel_format": "i420", **kw}),
    }
    bad_frames = [torch.zeros(2, 8, 10, 3, dtype=torch.uint8),               # RGB24 frames under a planar format
                  torch.zeros(2, 13, 10, dtype=torch.uint8),                 # rows no multiple of 3: no h with 3h/2 rows (odd h among them)
                  torch.zeros(2, 12, 9, dtype=torch.uint8),                  # odd w
                  torch.zeros(12, 10, dtype=torch.uint8),                    # one frame without the frame axis
                  torch.zeros(2, 12, 10, dtype=torch.float32),               # float frames
                  torch.zeros(2, 12, 10, dtype=torch.int16)]
    for name, call in calls.items():
        for fr in bad_frames:
            with pytest.raises(ValueError):
                call(fr)
        with pytest.raises(ValueError, match="pixel_format"):
            call(good, pixel_format="yuv444")
        with pytest.raises(ValueError, match="yuv_matrix"):
            call(good, yuv_matrix="bt2020")
        with pytest.raises(ValueError, match="yuv_range"):
            call(good, yuv_range="tv")
    with pytest.raises(ValueError, match="pixel_format"):
        video.yuv420_to_rgb(good, "rgb24")                                    # nothing to convert
    # planar frames with size: crop, resample and size are still checked before anything runs
    with pytest.raises(ValueError, match="outside"):
        calls["stylize_clip size"](good, crop=(4, 4, 8, 8))
    with pytest.raises(ValueError, match="resample"):
        video.resize_frames(good, (4, 4), None, "box", pixel_format="nv12")
    with pytest.raises(ValueError, match="crop"):
        calls["stylize_clip_conditioned"](good, crop="dyn")
    with pytest.raises(TypeError):
        ops.yuv420_to_rgb_host(good.float(), "i420")
    with pytest.raises(ValueError):
        ops.yuv420_to_rgb_host(good, "rgb24")
    with pytest.raises(ValueError, match="outside"):
        ops.yuv420_to_rgb_host(good, "i420", crop=(0, 0, 11, 8))
    # rgb24 callers are untouched: the default keeps refusing what it refused
    with pytest.raises(ValueError):
        video.stylize_clip(m, good, step_n=1)


def test_c_refusals(ops):
    """Every refusal of the two launching entry points that needs no device: checked before the launch, so bare addresses do."""
    from ncahip import _capi
    L = ops.lib()
    src, dst, ws, tab = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x800000), ctypes.c_void_p(0x1000000), ctypes.c_void_p(0x2000000)
    k = (ctypes.c_int32 * 6)(*COEFFS[("bt709", "limited")])
    conv = lambda **kw: L.ncahip_clip_yuv420_to_rgb_u8(*[{**dict(src=src, layout=0, N=2, H=8, W=10, x0=1, y0=1, cw=5, ch=3, k=k, dst=dst, stream=None),  # noqa: E731
                                                         **kw}[n] for n in ("src", "layout", "N", "H", "W", "x0", "y0", "cw", "ch", "k", "dst", "stream")])
    for kw in [dict(src=None), dict(dst=None), dict(k=None), dict(layout=2), dict(layout=-1), dict(N=0), dict(H=0), dict(W=-2), dict(cw=0), dict(ch=-1),
               dict(dst=ctypes.c_void_p(0x10000 + 100))]:
        assert conv(**kw) == _capi.EINVAL, kw
    assert b"overlap" in L.ncahip_last_error()
    for kw in [dict(H=7), dict(W=9), dict(x0=-1), dict(y0=-1), dict(x0=6), dict(y0=6), dict(cw=11, x0=0), dict(ch=9, y0=0), dict(H=16386), dict(W=16386),
               dict(x0=2 ** 31 - 1)]:
        assert conv(**kw) == _capi.ERANGE, kw

    def fused(**kw):
        a = {**dict(src=src, layout=1, k=k, N=2, H=8, W=10, x0=1, y0=1, cw=5, ch=3, kx=tab, bx=tab, ksx=5, ky=tab, by=tab, ksy=5, dst=dst, out_h=4,
                    out_w=4, ws=ws, ws_bytes=2 * 3 * 4 * 3, stream=None), **kw}
        return L.ncahip_clip_resize_yuv420_u8(*[a[n] for n in ("src", "layout", "k", "N", "H", "W", "x0", "y0", "cw", "ch", "kx", "bx", "ksx", "ky", "by",
                                                               "ksy", "dst", "out_h", "out_w", "ws", "ws_bytes", "stream")])
    for kw in [dict(src=None), dict(dst=None), dict(k=None), dict(layout=2), dict(N=0), dict(out_h=0), dict(ksx=0), dict(ws_bytes=2 * 3 * 4 * 3 - 1),
               dict(dst=ctypes.c_void_p(0x10000 + 100)), dict(ws=ctypes.c_void_p(0x10000 + 100))]:
        assert fused(**kw) == _capi.EINVAL, kw
    for kw in [dict(H=7), dict(W=9), dict(x0=6), dict(ch=9, y0=0), dict(H=16386), dict(out_w=16385), dict(ksx=2049), dict(kx=None), dict(by=None),
               dict(kx=ctypes.c_void_p(0x2000001)), dict(ws=None), dict(ws=ctypes.c_void_p(0x1000002))]:
        assert fused(**kw) == _capi.ERANGE, kw


@pytest.mark.parametrize("filt", ("bicubic", "lanczos"))
def test_cpu_route_equals_pillow_on_the_mirrors_rgb(ops, filt):
    Image = pytest.importorskip("PIL.Image")
    from ncahip import video
    pil_filter = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    gen = np.random.default_rng(11)
    for (h, w), size in [((36, 64), (16, 16)), ((20, 24), (40, 48)), ((40, 200), (8, 130))]:
        Y, U, V = planes(gen, 2, h, w)
        Y[1] = (Y[1] > 127) * np.uint8(255)
        for fmt, (matrix, rng) in zip(FORMATS, (("bt709", "limited"), ("bt601", "full"))):
            frames = torch.from_numpy(pack(Y, U, V, fmt))
            rgb = ops.yuv420_to_rgb_host(frames.numpy(), fmt, matrix, rng)
            for crop in (None, "dynca", "conditioned", (3, 1, 17, 15)):
                x0, y0, cw, ch = (0, 0, w, h) if crop is None else video.reference_crop(crop, h, w) if isinstance(crop, str) else crop
                want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(f[y0:y0 + ch, x0:x0 + cw])).resize((size[1], size[0]), pil_filter))
                                 for f in rgb])
                got = video.resize_frames(frames, size, crop, filt, pixel_format=fmt, yuv_matrix=matrix, yuv_range=rng)
                assert got.dtype == torch.uint8 and not got.is_cuda and np.array_equal(got.numpy(), want), (h, w, size, fmt, crop)
