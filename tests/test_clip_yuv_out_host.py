"""Host-side checks of planar YUV 4:2:0 images out of the clip calls (no GPU): the coefficients of ncahip_rgb_yuv_coeffs, the header's macro,
ops.rgb_to_yuv420_host -- the integer contract of include/ncahip.h in numpy -- against an independent float64 evaluation of the real-valued
definition over all 2^24 flat colours and 2^22 random channel sums, the two layouts, the refusals of the C and Python entry points, and the
loop route of stylize_clip on CPU tensors with out_format= and out=.  Every C call here fails a host-side check: no pointer is dereferenced."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("i420", "nv12")
MODES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
# the issue's table: (R, G, B) rows of Y, U, V, then the luma offset
COEFFS = {("bt601", "limited"): (16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681, 16),
          ("bt601", "full"): (19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329, 0),
          ("bt709", "limited"): (11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639, 16),
          ("bt709", "full"): (13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005, 0)}
NEW = {"ncahip_rgb_yuv_coeffs": 3, "ncahip_clip_rgb_to_yuv420_u8": 8}


@pytest.fixture(scope="module")
def ops():
    from ncahip import ops as _ops
    return _ops


def P(a):
    return ctypes.c_void_p(a)


def fmt_word(layout, matrix, rng):
    return 0x100 | layout | matrix << 1 | rng << 2


def test_coefficients(ops):
    from ncahip import _capi
    L = ops.lib()
    for (matrix, rng), want in COEFFS.items():
        k = (ctypes.c_int32 * 10)()
        assert L.ncahip_rgb_yuv_coeffs(_capi.YUV_MATRICES[matrix], _capi.YUV_RANGES[rng], k) == 0
        assert tuple(k) == want, (matrix, rng)
        assert sum(want[0:3]) == (56284 if rng == "limited" else 65536) and sum(want[3:6]) == 0 and sum(want[6:9]) == 0
        got = ops.rgb_yuv_coeffs(matrix, rng)
        assert got.dtype == np.int32 and tuple(int(v) for v in got) == want and ops.rgb_yuv_coeffs(matrix, rng) is got      # cached
        assert not got.flags.writeable
    k = (ctypes.c_int32 * 10)()
    for matrix, rng in [(2, 0), (-1, 0), (0, 2), (0, -1)]:
        assert L.ncahip_rgb_yuv_coeffs(matrix, rng, k) == _capi.EINVAL
    assert L.ncahip_rgb_yuv_coeffs(0, 0, None) == _capi.EINVAL
    with pytest.raises(ValueError, match="yuv_matrix"):
        ops.rgb_yuv_coeffs("bt2020", "full")
    with pytest.raises(ValueError, match="yuv_range"):
        ops.rgb_yuv_coeffs("bt709", "tv")


def test_header_macro_exports_and_signatures(ops):
    from ncahip import _capi
    hdr = open(os.path.join(ROOT, "include", "ncahip.h")).read()
    assert "#define NCAHIP_CLIP_YUV420(layout, matrix, range) (0x100 | (layout) | (matrix) << 1 | (range) << 2)" in hdr
    assert "#define NCAHIP_CLIP_F32_NCHW 0 " in hdr and "#define NCAHIP_CLIP_U8_NHWC  1 " in hdr          # the two old lines stay
    words = sorted(_capi.clip_yuv420(la, m, r) for la in (0, 1) for m in (0, 1) for r in (0, 1))
    assert words == list(range(0x100, 0x108)) and words == sorted(fmt_word(la, m, r) for la in (0, 1) for m in (0, 1) for r in (0, 1))
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
              for m in re.finditer(r"\b(?:int|size_t)\s*(ncahip_\w+)\s*\(([^)]*)\)\s*;", src)}
    raw = ctypes.CDLL(_capi.LIB_PATH)
    L = ops.lib()
    for name, nargs in NEW.items():
        assert hasattr(raw, name) and protos.get(name) == nargs and len(_capi.SIGNATURES[name]) == nargs, name
        assert getattr(L, name).argtypes is not None


def real_valued(rgb, sums, matrix, rng):
    """The real-valued definition in float64, rounded half up (not clamped): Y of pixels [..., 3], (U, V) of 2 x 2 channel sums [..., 3]."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    sy, sc, off = (219.0 / 255.0, 224.0 / 255.0, 16.0) if rng == "limited" else (1.0, 1.0, 0.0)
    rgb, mean = rgb.astype(np.float64), sums.astype(np.float64) / 4.0
    luma = lambda c: kr * c[..., 0] + kg * c[..., 1] + kb * c[..., 2]      # noqa: E731
    Y = off + sy * luma(rgb)
    U = 128.0 + sc * (mean[..., 2] - luma(mean)) / (2.0 * (1.0 - kb))
    V = 128.0 + sc * (mean[..., 0] - luma(mean)) / (2.0 * (1.0 - kr))
    return tuple(np.floor(p + 0.5).astype(np.int64) for p in (Y, U, V))


@pytest.mark.parametrize("matrix,rng", MODES)
def test_mirror_against_float64(ops, matrix, rng):
    """All 2^24 flat colours (a flat 2 x 2 block: sums = 4 * colour) and 2^22 seeded random channel-sum triples: the integer contract is never
    more than 1 away from the real-valued definition rounded half up and differs from it on at most 7.7e-4 of a plane's values; limited range stays inside [16, 235] / [16, 240]; grey gives 128."""
    k = ops.rgb_yuv_coeffs(matrix, rng)
    gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2)
    worst, differing, total = 0, np.zeros(3), 0
    lo, hi = np.full(3, 255), np.zeros(3, dtype=np.int64)
    for r0 in range(0, 256, 16):
        rgb = np.concatenate([np.concatenate((np.full((gb.shape[0], 1), r), gb), axis=1) for r in range(r0, r0 + 16)]).astype(np.int32)
        got = ops.rgb_yuv_planes_host(rgb, 4 * rgb, k)
        want = real_valued(rgb, 4 * rgb, matrix, rng)
        for i in range(3):
            d = np.abs(got[i].astype(np.int64) - np.clip(want[i], 0, 255))
            worst, differing[i] = max(worst, int(d.max())), differing[i] + int((d != 0).sum())
            lo[i], hi[i] = min(lo[i], int(got[i].min())), max(hi[i], int(got[i].max()))
        total += rgb.shape[0]
    assert total == 1 << 24
    sums = np.random.default_rng(20).integers(0, 1021, (1 << 22, 3)).astype(np.int32)
    _, U, V = ops.rgb_yuv_planes_host(np.zeros_like(sums), sums, k)
    _, wu, wv = real_valued(np.zeros_like(sums), sums, matrix, rng)
    du, dv = np.abs(U.astype(np.int64) - np.clip(wu, 0, 255)), np.abs(V.astype(np.int64) - np.clip(wv, 0, 255))
    worst = max(worst, int(du.max()), int(dv.max()))
    frac = [float(differing[i]) / total for i in range(3)] + [float((du != 0).mean()), float((dv != 0).mean())]
    print(f"{matrix} {rng}: max |diff| {worst}, differing fraction (Y, U, V flat; U, V random sums) {frac}, ranges {list(zip(lo, hi))}")
    assert worst <= 1
    assert max(frac) <= 7.7e-4, frac                             # the contract's bound (include/ncahip.h); the worst is bt709 limited, U
    if rng == "limited":
        assert (lo[0], hi[0]) == (16, 235) and (lo[1], hi[1]) == (16, 240) and (lo[2], hi[2]) == (16, 240)
        assert 16 <= int(min(U.min(), V.min())) and int(max(U.max(), V.max())) <= 240
    else:
        assert (lo[0], hi[0]) == (0, 255)
    grey = np.repeat(np.arange(256, dtype=np.int32)[:, None], 3, axis=1)
    _, U, V = ops.rgb_yuv_planes_host(grey, 4 * grey, k)
    assert (U == 128).all() and (V == 128).all()
    # a grey block whose four pixels differ gives 128 as well: the rows sum to 0 exactly
    s = np.repeat(np.arange(0, 1021, dtype=np.int32)[:, None], 3, axis=1)
    _, U, V = ops.rgb_yuv_planes_host(np.zeros_like(s), s, k)
    assert (U == 128).all() and (V == 128).all()


@pytest.mark.parametrize("matrix,rng", MODES)
def test_layouts_hold_the_same_samples(ops, matrix, rng):
    from ncahip import video
    gen = np.random.default_rng(5)
    k = ops.rgb_yuv_coeffs(matrix, rng)
    for h, w in [(2, 2), (6, 6), (6, 10), (18, 66)]:
        rgb = gen.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
        rgb[1] = (rgb[1] > 127) * np.uint8(255)
        a = ops.rgb_to_yuv420_host(rgb, "i420", matrix, rng)
        b = ops.rgb_to_yuv420_host(rgb, "nv12", matrix, rng)
        assert a.dtype == np.uint8 and a.shape == b.shape == (2, 3 * h // 2, w)
        a, b = a.reshape(2, -1), b.reshape(2, -1)
        assert np.array_equal(a[:, :h * w], b[:, :h * w])
        U, V = a[:, h * w:h * w + h * w // 4], a[:, h * w + h * w // 4:]
        assert np.array_equal(np.stack((U, V), axis=-1).reshape(2, -1), b[:, h * w:])
        # the planes are the contract applied to the pixels and to the 2 x 2 sums
        i = rgb.astype(np.int32)
        Y, U2, V2 = ops.rgb_yuv_planes_host(i, i[:, 0::2, 0::2] + i[:, 0::2, 1::2] + i[:, 1::2, 0::2] + i[:, 1::2, 1::2], k)
        assert np.array_equal(Y.reshape(2, -1), a[:, :h * w]) and np.array_equal(U2.reshape(2, -1), U) and np.array_equal(V2.reshape(2, -1), V)
    t = torch.from_numpy(rgb)
    got = video.rgb_to_yuv420(t, "nv12", matrix, rng)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and np.array_equal(got.numpy().reshape(2, -1), b)


def test_c_refusals_of_the_conversion(ops):
    from ncahip import _capi
    L = ops.lib()
    k = (ctypes.c_int32 * 10)(*COEFFS[("bt709", "limited")])
    base = dict(src=P(0x10000), layout=0, N=2, H=8, W=10, k=k, dst=P(0x800000), stream=None)
    conv = lambda **kw: L.ncahip_clip_rgb_to_yuv420_u8(*[{**base, **kw}[n] for n in ("src", "layout", "N", "H", "W", "k", "dst", "stream")])  # noqa: E731
    for kw in [dict(src=None), dict(dst=None), dict(k=None), dict(layout=2), dict(layout=-1), dict(N=0), dict(H=0), dict(W=-2),
               dict(dst=P(0x10000 + 2 * 8 * 10 * 3 - 1)), dict(dst=P(0x10000 - 2 * 12 * 10 + 1))]:      # the last byte of src / of dst
        assert conv(**kw) == _capi.EINVAL, kw
    assert b"overlap" in L.ncahip_last_error()
    for kw in [dict(H=7), dict(W=9), dict(H=16386), dict(W=16386)]:
        assert conv(**kw) == _capi.ERANGE, kw


def emit_calls(L):
    """The six entry points that take an image format, with fake pointers: name -> call(**overrides).  Every use below overrides something
    that a host-side check refuses, so nothing is launched.  The drivers take ws=<pointer>: a persistent workspace with epoch0 = 0, which
    the epoch check -- the one after the overlap check -- refuses."""
    st, img, gray = 0x1000000, 0x3000000, 0x2000000

    def emit(**kw):
        a = dict(dict(st=P(st), img=P(img), fmt=0, B=1, C=12, c_out=3, H=8, W=8), **kw)
        return L.ncahip_clip_emit(a["st"], a["img"], a["fmt"], a["B"], a["C"], a["c_out"], a["H"], a["W"], None)

    def inject(**kw):
        a = dict(dict(st=P(st), img=P(img), fmt=0, gray=P(gray), B=1, C=12, c_out=3, H=8, W=8), **kw)
        return L.ncahip_clip_emit_inject(a["st"], a["img"], a["fmt"], a["gray"], a["B"], a["C"], a["c_out"], a["H"], a["W"], None)

    def unit(**kw):
        a = dict(dict(st=P(st), img=P(img), fmt=0, B=1, C=16, c_out=3, H=8, W=8), **kw)
        return L.ncahip_clip_emit_unit(a["st"], a["img"], a["fmt"], a["B"], a["C"], a["H"], a["W"], None)

    w = dict(w1=P(0x4000000), b1=P(0x4100000), w2=P(0x4200000), b2=P(0x4300000))

    def dynca(**kw):
        a = dict(dict(st=P(st), cond=P(gray), img=P(img), fmt=0, F=3, k=2, B=1, C=12, c_out=3, H=8, W=8, **w), **kw)
        return L.ncahip_dynca_clip_f32(a["st"], a["cond"], a["img"], a["fmt"], a["F"], a["k"], 4, None, a["w1"], a["b1"], a["w2"], a["b2"], a["B"], a["C"],
                                       a["c_out"], a["H"], a["W"], 96, 1, 0, 0.5, 0, 0, None, a.get("ws"), 1 << 30, 0, None)

    def xc(**kw):
        a = dict(dict(st=P(st), cond=None, img=P(img), fmt=0, F=3, k=2, B=1, C=13, c_out=3, H=8, W=8, **w), **kw)
        return L.ncahip_dynca_clip_xc_f32(a["st"], P(gray), a["cond"], 0, a["img"], a["fmt"], a["F"], a["k"], 4, None, a["w1"], a["b1"], a["w2"], a["b2"],
                                          a["B"], a["C"], a["c_out"], a["H"], a["W"], 96, 1, 0, 0.5, 0, 0, None, a.get("ws"), 1 << 30, 0, None)

    def cond(**kw):
        a = dict(dict(st=P(st), img=P(img), fmt=0, F=3, k=2, B=1, C=16, c_out=3, H=8, W=8), **kw)
        return L.ncahip_cond_clip_f32(a["st"], P(0x5000000), P(gray), 12, a["img"], a["fmt"], a["F"], a["k"], 4, None, P(0x4000000), P(0x4100000),
                                      P(0x4200000), P(0x4300000), P(0x4400000), P(0x4500000), a["B"], a["C"], a["H"], a["W"], 64, 3, 0.1, 0.5, -10.0, 10.0,
                                      0, 0, a.get("ws"), 1 << 30, 0, None)

    return {"emit": emit, "emit_inject": inject, "emit_unit": unit, "dynca_clip": dynca, "dynca_clip_xc": xc, "cond_clip": cond}, st, img


def test_c_image_formats(ops):
    """0x100 .. 0x107 are image formats of the three emits and the three drivers: accepted up to the next check (here: the overlap check, with
    the planar image's size), c_out != 3 and odd sides refused, every other unknown value still 'format'."""
    from ncahip import _capi
    L = ops.lib()
    calls, st, img = emit_calls(L)
    H = W = 8
    for name, call in calls.items():
        n_img = 1 if name.startswith("emit") else 6
        planar = n_img * 3 * H * W // 2
        for fmt in range(0x100, 0x108):
            # the image overlapping the state is the next check: refused with 'overlap', not with 'format'
            assert call(fmt=fmt, img=P(st)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error(), (name, hex(fmt))
            # the last byte of the planar image lies on the first byte of the state: refused
            assert call(fmt=fmt, img=P(st - planar + 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error(), (name, hex(fmt))
            for kw in (dict(H=7), dict(W=6 + 1), dict(H=9, W=9)):
                assert call(fmt=fmt, **kw) == _capi.ERANGE and b"even" in L.ncahip_last_error(), (name, hex(fmt), kw)
            if name not in ("emit_unit", "cond_clip"):
                for c_out in (1, 2, 4):
                    assert call(fmt=fmt, c_out=c_out) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error(), (name, hex(fmt), c_out)
        # one byte lower the planar images end before the state: the drivers go on to the next check (the epochs), while the uint8 RGB
        # images, twice as long, still overlap there
        if n_img > 1:
            assert call(fmt=0x103, img=P(st - planar), ws=P(0x6000000)) == _capi.EINVAL and b"epoch" in L.ncahip_last_error(), name
            assert call(fmt=1, img=P(st - planar), ws=P(0x6000000)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error(), name
        for fmt in (2, 7, -1, 0x108, 0xff, 0x200, 0x1100):
            assert call(fmt=fmt) == _capi.EINVAL and b"format" in L.ncahip_last_error(), (name, fmt)


def test_c_frame_formats_stay_refused(ops):
    from ncahip import _capi
    L = ops.lib()
    fr, k3, out = P(0x100000), P(0x200000), P(0x300000)
    for fmt in list(range(0x100, 0x108)) + [2, 7, -1]:
        assert L.ncahip_clip_cond(fr, fmt, k3, 1 / 3, 1 / 3, 1 / 3, 1, out, 2, 1, 8, 8, None) == _capi.EINVAL and b"format" in L.ncahip_last_error()
        assert L.ncahip_clip_gray(fr, fmt, 1 / 3, 1 / 3, 1 / 3, out, 2, 1, 8, 8, None) == _capi.EINVAL and b"format" in L.ncahip_last_error()
        assert L.ncahip_clip_encode(fr, fmt, k3, k3, k3, k3, k3, out, 2, 1, 3, 16, 8, 8, None) == _capi.EINVAL and b"format" in L.ncahip_last_error()


class _HostModel:
    """The surface stylize_clip's loop route uses, in torch ops on the host (the DyNCA drop-in itself has no CPU path)."""
    device = torch.device("cpu")
    conditioning = "edges"
    perception_scales = [0]
    c_in, c_out = 6, 3
    _mask_step = 0

    def seed(self, n, size=128):
        sx, sy = (size, size) if isinstance(size, int) else size
        return torch.zeros(n, self.c_in, sy, sx)

    def forward_nsteps(self, h, step_n, cond_img=None):
        self._mask_step += step_n
        h = h + 0.05 * step_n * (cond_img + 0.5)
        return h, h[:, :self.c_out] * 2.0 + torch.linspace(-1.5, 1.5, h.shape[-1])


def test_python_refusals_on_cpu_tensors(ops):
    from ncahip import video
    from ncahip.nca import ConditionedNCA
    frames = torch.zeros(2, 8, 10, 3, dtype=torch.uint8)
    nca = ConditionedNCA(target_shape=(3, 8, 8), num_hidden_channels=4)
    calls = {"stylize_clip": lambda fr=frames, **kw: video.stylize_clip(_HostModel(), fr, step_n=1, **{"out_dtype": torch.uint8, **kw}),
             "conditioned": lambda fr=frames[:, :, :8], **kw: video.stylize_clip_conditioned(nca, fr, step_n=1, **{"out_dtype": torch.uint8, **kw})}
    for name, call in calls.items():
        with pytest.raises(ValueError, match="out_format"):
            call(out_format="yuv444")
        with pytest.raises(ValueError, match="yuv_matrix"):
            call(out_format="i420", out_yuv_matrix="bt2020")
        with pytest.raises(ValueError, match="yuv_range"):
            call(out_format="nv12", out_yuv_range="tv")
        with pytest.raises(ValueError, match="uint8"):
            call(out_format="i420", out_dtype=torch.float32)
        with pytest.raises(ValueError, match="even"):
            call(frames[:, :7, :8] if name == "conditioned" else frames[:, :7], out_format="i420", **({"state": torch.zeros(1, 8, 7, 8)} if name == "conditioned" else {}))
        with pytest.raises(ValueError, match="even"):
            call(frames[:, :8, :7] if name == "conditioned" else frames[:, :, :9], out_format="nv12", **({"state": torch.zeros(1, 8, 8, 7)} if name == "conditioned" else {}))
        h, w = (8, 8) if name == "conditioned" else (8, 10)
        for bad in (torch.zeros(2, h, w, 3, dtype=torch.uint8),                       # RGB-shaped out under a planar format
                    torch.zeros(3, 3 * h // 2, w, dtype=torch.uint8),                 # one image too many
                    torch.zeros(2, 3 * h // 2, w, dtype=torch.float32),               # dtype
                    torch.zeros(2, 3 * h // 2, 2 * w, dtype=torch.uint8)[:, :, ::2],  # not contiguous
                    "images"):
            with pytest.raises(ValueError, match="out must be"):
                call(out_format="i420", out=bad)
        with pytest.raises(ValueError, match="out must be"):
            call(out=torch.zeros(2, 3 * h // 2, w, dtype=torch.uint8))                # planar-shaped out under rgb24
    m = _HostModel()
    m.c_out = 4
    with pytest.raises(ValueError, match="c_out"):
        video.stylize_clip(m, frames, step_n=1, out_dtype=torch.uint8, out_format="i420")
    # a refused out leaves the model's fire-mask position where it was
    m = _HostModel()
    m._mask_step = 40
    with pytest.raises(ValueError):
        video.stylize_clip(m, frames, step_n=1, out_dtype=torch.uint8, out_format="i420", out=torch.zeros(1, 12, 10, dtype=torch.uint8))
    assert m._mask_step == 40
    for fn in (video.rgb_to_yuv420, ):
        with pytest.raises(ValueError, match="pixel_format"):
            fn(frames, "rgb24")
        with pytest.raises(ValueError):
            fn(frames.float(), "i420")
        with pytest.raises(ValueError, match="even"):
            fn(frames[:, :7], "i420")
        with pytest.raises(ValueError):
            fn(frames[0], "i420")
    with pytest.raises(TypeError):
        ops.rgb_to_yuv420_host(frames.float(), "i420")
    with pytest.raises(ValueError, match="out_format"):
        ops._clip_img_fmt(torch.uint8, "yuv444")
    with pytest.raises(ValueError, match="uint8"):
        ops._clip_img_fmt(torch.float32, "i420")
    assert ops._clip_img_fmt(torch.uint8, "nv12", "bt709", "full", 3, 8, 8) == fmt_word(1, 1, 1)
    assert ops._clip_img_fmt(torch.uint8) == 1 and ops._clip_img_fmt(torch.float32) == 0


@pytest.mark.parametrize("fmt,mode", [("i420", ("bt709", "limited")), ("nv12", ("bt601", "full"))])
def test_loop_route_on_a_cpu_model_gives_the_mirror_of_its_rgb_images(ops, fmt, mode):
    from ncahip import video
    u8 = torch.randint(0, 256, (3, 6, 10, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    rgb, s_rgb = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2, out_dtype=torch.uint8)
    assert video.stylize_clip.last_path == "loop" and video.stylize_clip.last_download is None
    assert 0 < int(rgb.min()) + 1 and int(rgb.max()) == 255 and len(torch.unique(rgb)) > 50                # a real image, both clamps near
    want = ops.rgb_to_yuv420_host(rgb, fmt, *mode)
    kw = dict(out_format=fmt, out_yuv_matrix=mode[0], out_yuv_range=mode[1])
    for per_call in (1, 2, 32):
        got, s = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2, out_dtype=torch.uint8, frames_per_call=per_call, **kw)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (6, 9, 10) and torch.equal(got, want) and torch.equal(s, s_rgb)
        assert video.stylize_clip.last_download is None
        out = torch.full((6, 9, 10), 77, dtype=torch.uint8)
        ret, s = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2, out_dtype=torch.uint8, frames_per_call=per_call, out=out, **kw)
        assert ret is out and torch.equal(out, want) and torch.equal(s, s_rgb) and video.stylize_clip.last_download == "sync"
    # out= with the default format, float32 and uint8
    out = torch.zeros_like(rgb)
    ret, _ = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2, out_dtype=torch.uint8, out=out, frames_per_call=2)
    assert ret is out and torch.equal(out, rgb)
    f32, _ = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2)
    out = torch.zeros_like(f32)
    ret, _ = video.stylize_clip(_HostModel(), u8, step_n=2, steps_per_frame=2, out=out)
    assert ret is out and torch.equal(out, f32)
    # no frames: an empty planar clip
    got, _ = video.stylize_clip(_HostModel(), u8[:0], step_n=2, out_dtype=torch.uint8, **kw)
    assert tuple(got.shape) == (0, 9, 10) and got.dtype == torch.uint8
