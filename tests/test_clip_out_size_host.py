"""Host-side checks of images at delivery size (no GPU): ops.clip_resize_host enlarging against Pillow and the fixture
tests/golden/g13_clip_upscale.npz, ops.clip_resize_to_yuv420_host (the composition that defines ncahip_clip_resize_u8_yuv420),
video.resize_frames(out_format=...) on CPU tensors, out_size= / out_resample= of stylize_clip and stylize_clip_conditioned on CPU models
(the loop route), every refusal before a model step runs, and the new symbol.  Every comparison is exact."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ("bicubic", "lanczos")
GRID, OUT_SIZE, F, K, STEP_N, PER_CALL = (16, 24), (36, 52), 3, 1, 2, 2
SYMBOL, NARGS = "ncahip_clip_resize_u8_yuv420", 22


@pytest.fixture(scope="module")
def ops():
    from ncahip import _capi, ops as _ops
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ops


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g13_clip_upscale.npz"))


def _cases(g):
    for c in range(len(g["case_input"])):
        yield c, g[f"in_{int(g['case_input'][c])}"], tuple(int(v) for v in g["case_size"][c]), str(g["case_filter"][c]), g[f"out_{c}"]


def _checker(h=16, w=24):
    img = np.zeros((h, w, 3), dtype=np.uint8)
    img[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = 255
    return img


# ------------------------------------------------------------------ 1. the mirror's RGB half: Pillow and the fixture
def test_rgb_mirror_equals_the_fixture(ops, golden):
    n = 0
    for c, img, size, filt, want in _cases(golden):
        assert img.shape[0] <= 24 and img.shape[1] <= 32
        got = ops.clip_resize_host(img[None], size, None, filt)
        assert got.dtype == np.uint8 and np.array_equal(got[0], want), (c, size, filt)
        n += 1
    assert n >= 8 and {str(f) for f in golden["case_filter"]} == set(FILTERS)


def test_rgb_mirror_equals_pillow_directly(ops, golden):
    from PIL import Image                              # a missing Pillow is a failure here; the fixture test above needs none
    pil = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    rng = np.random.default_rng(31)
    shapes = [((10, 14), (22, 30)), ((16, 24), (36, 52)), ((9, 7), (18, 14)), ((20, 24), (20, 24)), ((4, 6), (6, 6)), ((16, 32), (36, 68)),
              ((15, 32), (36, 68))]
    for (h, w), size in shapes:
        for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), _checker(h, w)):
            for filt in FILTERS:
                want = np.asarray(Image.fromarray(img).resize((size[1], size[0]), pil[filt]))
                assert np.array_equal(ops.clip_resize_host(img[None], size, None, filt)[0], want), ((h, w), size, filt)
    # the fixture is what this Pillow returns today
    for c, img, size, filt, want in _cases(golden):
        assert np.array_equal(np.asarray(Image.fromarray(img).resize((size[1], size[0]), pil[filt])), want), c


# ------------------------------------------------------------------ 2. the planar mirror is the composition
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_planar_mirror_is_the_composition(ops, golden, fmt):
    for matrix, rng in [("bt709", "limited"), ("bt601", "full")]:
        for c, img, size, filt, want in _cases(golden):
            got = ops.clip_resize_to_yuv420_host(img[None], size, None, filt, fmt, matrix, rng)
            assert got.dtype == np.uint8 and got.shape == (1, 3 * size[0] // 2, size[1])
            assert np.array_equal(got, ops.rgb_to_yuv420_host(want[None], fmt, matrix, rng)), (c, fmt, matrix, rng)
    # a crop box, tensors in and out
    t = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (2, 20, 24, 3), dtype=np.uint8))
    got = ops.clip_resize_to_yuv420_host(t, (30, 22), (3, 1, 17, 15), "lanczos", fmt)
    assert isinstance(got, torch.Tensor) and torch.equal(got, ops.rgb_to_yuv420_host(ops.clip_resize_host(t, (30, 22), (3, 1, 17, 15), "lanczos"), fmt))
    for size in ((21, 30), (22, 29)):
        with pytest.raises(ValueError, match="even"):
            ops.clip_resize_to_yuv420_host(t, size, None, "bicubic", fmt)
    with pytest.raises(ValueError, match="pixel_format"):
        ops.clip_resize_to_yuv420_host(t, (22, 30), None, "bicubic", "rgb24")
    with pytest.raises(ValueError, match="resample"):
        ops.clip_resize_to_yuv420_host(t, (22, 30), None, "cubic", fmt)


def test_chroma_from_unclamped_accumulators_differs(ops):
    """Negative control on the mirror: the RGB bytes are clamped after the vertical pass's >> 22, BEFORE any YUV arithmetic.  Chroma formed
    from the un-clamped values (bicubic overshoot on the 0 / 255 image) is a different image."""
    img = _checker()
    img[:, :, 1] = 255 - img[:, :, 1]                                  # coloured: chroma away from 128
    size, filt = OUT_SIZE, "bicubic"
    kx, bx = ops.resize_tables(img.shape[1], size[1], filt)
    ky, by = ops.resize_tables(img.shape[0], size[0], filt)
    tmp = ops._resize_pass_host(img[None], kx, bx, axis=2)              # uint8 between the passes, as the contract has it
    raw = np.empty((1, size[0], size[1], 3), dtype=np.int32)            # the vertical pass without its clamp
    t32 = tmp.astype(np.int32)
    for i in range(size[0]):
        y, n = int(by[i, 0]), int(by[i, 1])
        raw[:, i] = (np.tensordot(t32[:, y:y + n], ky[i, :n].astype(np.int32), axes=([1], [0])) + (1 << 21)) >> 22
    assert np.array_equal(np.clip(raw, 0, 255).astype(np.uint8), ops.clip_resize_host(img[None], size, None, filt))
    assert raw.min() < 0 and raw.max() > 255                           # the overshoot is there
    k = ops.rgb_yuv_coeffs("bt709", "full")
    block = lambda a: a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]      # noqa: E731
    clamped = np.clip(raw, 0, 255)
    _, u_good, v_good = ops.rgb_yuv_planes_host(clamped, block(clamped), k)
    _, u_bad, v_bad = ops.rgb_yuv_planes_host(clamped, block(raw), k)
    want = ops.clip_resize_to_yuv420_host(img[None], size, None, filt, "i420", "bt709", "full").reshape(1, -1)
    hw = size[0] * size[1]
    assert np.array_equal(want[:, hw:hw + hw // 4], u_good.reshape(1, -1)) and np.array_equal(want[:, hw + hw // 4:], v_good.reshape(1, -1))
    assert not np.array_equal(u_bad, u_good) or not np.array_equal(v_bad, v_good)


# ------------------------------------------------------------------ 3. resize_frames(out_format=...) on CPU tensors
def test_resize_frames_out_format_on_cpu_tensors(ops):
    from ncahip import video
    t = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (2, 20, 24, 3), dtype=np.uint8))
    rgb = video.resize_frames(t, (30, 44), "dynca", "lanczos")
    assert torch.equal(video.resize_frames(t, (30, 44), "dynca", "lanczos", out_format="rgb24"), rgb)            # the default
    for fmt in ("i420", "nv12"):
        got = video.resize_frames(t, (30, 44), "dynca", "lanczos", out_format=fmt, out_yuv_matrix="bt601", out_yuv_range="full")
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 45, 44)
        assert torch.equal(got, video.rgb_to_yuv420(rgb, fmt, "bt601", "full"))
    # planar frames in, planar images out: the conversion of the resized image
    planar = video.rgb_to_yuv420(t, "nv12")
    got = video.resize_frames(planar, (30, 44), None, "bicubic", pixel_format="nv12", out_format="i420")
    assert torch.equal(got, video.rgb_to_yuv420(video.resize_frames(planar, (30, 44), None, "bicubic", pixel_format="nv12"), "i420"))
    with pytest.raises(ValueError, match="out_format"):
        video.resize_frames(t, (30, 44), out_format="yuv444")
    with pytest.raises(ValueError, match="even"):
        video.resize_frames(t, (31, 44), out_format="i420")
    with pytest.raises(ValueError, match="yuv_matrix"):
        video.resize_frames(t, (30, 44), out_format="i420", out_yuv_matrix="bt2020")
    with pytest.raises(ValueError, match="frames must be"):
        video.resize_frames(t.float(), (30, 44), out_format="i420")


# ------------------------------------------------------------------ 4. the clip calls on CPU models (the loop route)
class _HostModel:
    """The surface stylize_clip's loop route uses, in torch ops on the host (the DyNCA drop-in itself has no CPU path)."""
    device = torch.device("cpu")
    conditioning = "edges"
    perception_scales = [0]
    c_in, c_out = 6, 3

    def __init__(self):
        self._mask_step = 0

    def seed(self, n, size=128):
        sx, sy = (size, size) if isinstance(size, int) else size
        return torch.zeros(n, self.c_in, sy, sx)

    def forward_nsteps(self, h, step_n, cond_img=None):
        self._mask_step += step_n
        h = h + 0.05 * step_n * (cond_img + 0.5)
        return h, h[:, :self.c_out] * 2.0 + torch.linspace(-1.5, 1.5, h.shape[-1])


def _host_cond():
    """A tiny ConditionedNCA on the CPU (C = 3 + 1 + 4) whose grow is torch ops on the host; counts its grow calls."""
    from ncahip.nca import ConditionedNCA

    class HostCond(ConditionedNCA):
        calls = 0

        def grow(self, x, num_steps, goal):
            self.calls += 1
            return x + 0.04 * num_steps * (goal.mean(1, keepdim=True) - 0.2) + torch.linspace(-0.05, 0.05, x.shape[-1])

    return HostCond(target_shape=(3, GRID[0], GRID[0]), num_hidden_channels=4)


def _frames():
    return torch.randint(0, 256, (F,) + GRID + (3,), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)


def _entry(name):
    """call(**kw) -> (images, state, model) of one call of the entry point on a fresh CPU model."""
    from ncahip import video

    def call(**kw):
        kw = dict(dict(step_n=STEP_N, steps_per_frame=K, out_dtype=torch.uint8, frames_per_call=PER_CALL), **kw)
        if name == "stylize_clip":
            m = _HostModel()
            return video.stylize_clip(m, _frames(), **kw) + (m,)
        m = _host_cond()
        kw.setdefault("state", torch.zeros(1, m.num_channels, *GRID))
        return video.stylize_clip_conditioned(m, _frames(), **kw) + (m,)

    return call, getattr(video, name)


@pytest.mark.parametrize("fmt", ["rgb24", "i420"])
@pytest.mark.parametrize("name", ["stylize_clip", "stylize_clip_conditioned"])
def test_clip_calls_with_out_size_on_cpu_models(ops, name, fmt):
    from ncahip import video
    call, fn = _entry(name)
    plain, plain_state, _ = call()
    assert fn.last_path == "loop" and tuple(plain.shape) == (F * K,) + GRID + (3,) and len(torch.unique(plain)) > 20
    for resample in FILTERS:
        want = video.resize_frames(plain, OUT_SIZE, None, resample)
        shape = OUT_SIZE + (3,)
        if fmt != "rgb24":
            want, shape = video.rgb_to_yuv420(want, fmt), (3 * OUT_SIZE[0] // 2, OUT_SIZE[1])
        kw = dict(out_size=OUT_SIZE, out_resample=resample, out_format=fmt)
        for per_call in (PER_CALL, 1, 32):
            got, state, _ = call(frames_per_call=per_call, **kw)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (F * K,) + shape and fn.last_path == "loop" and fn.last_download is None
            assert torch.equal(got, want) and torch.equal(state, plain_state), (resample, per_call)
        out = torch.full((F * K,) + shape, 77, dtype=torch.uint8)                   # pageable
        got, state, _ = call(out=out, **kw)
        assert got is out and fn.last_download == "sync" and torch.equal(out, want) and torch.equal(state, plain_state)
    # bicubic is the default
    got, _, _ = call(out_size=OUT_SIZE, out_format=fmt)
    want = video.resize_frames(plain, OUT_SIZE, None, "bicubic", out_format=fmt)
    assert torch.equal(got, want)


def test_odd_grid_with_an_even_out_size_is_accepted_for_planar_output(ops):
    from ncahip import video
    frames = torch.randint(0, 256, (2, 15, 24, 3), generator=torch.Generator().manual_seed(8), dtype=torch.uint8)
    plain, _ = video.stylize_clip(_HostModel(), frames, step_n=1, out_dtype=torch.uint8)
    got, _ = video.stylize_clip(_HostModel(), frames, step_n=1, out_dtype=torch.uint8, out_size=OUT_SIZE, out_format="nv12")
    assert torch.equal(got, video.rgb_to_yuv420(video.resize_frames(plain, OUT_SIZE), "nv12"))
    with pytest.raises(ValueError, match="even"):                                    # without out_size the rule is the grid's
        video.stylize_clip(_HostModel(), frames, step_n=1, out_dtype=torch.uint8, out_format="nv12")
    empty, _ = video.stylize_clip(_HostModel(), frames[:0], step_n=1, out_dtype=torch.uint8, out_size=OUT_SIZE, out_format="nv12")
    assert tuple(empty.shape) == (0, 54, 52) and empty.dtype == torch.uint8


@pytest.mark.parametrize("name", ["stylize_clip", "stylize_clip_conditioned"])
def test_out_size_refusals_before_any_model_step(ops, name):
    call, _ = _entry(name)
    steps = lambda m: m._mask_step if name == "stylize_clip" else m.calls      # noqa: E731
    seen = []

    def refused(match, **kw):
        from ncahip import video
        m = _HostModel() if name == "stylize_clip" else _host_cond()
        kw = dict(dict(step_n=STEP_N, out_dtype=torch.uint8), **kw)
        if name != "stylize_clip":
            kw.setdefault("state", torch.zeros(1, m.num_channels, *GRID))
        with pytest.raises(ValueError, match=match):
            getattr(video, name)(m, _frames(), **kw)
        assert steps(m) == 0
        seen.append(match)

    refused("uint8", out_size=OUT_SIZE, out_dtype=torch.float32)
    for bad in ((36,), (36, 52, 3), 36, "big", (36, "w"), (36.5, 52)):
        refused("out_size must be", out_size=bad)
    for bad in ((0, 52), (36, -2)):
        refused("positive", out_size=bad)
    for bad in ("cubic", "nearest", None):
        refused("out_resample", out_size=OUT_SIZE, out_resample=bad)
    for bad, fmt in (((35, 52), "i420"), ((36, 51), "nv12")):
        refused("even", out_size=bad, out_format=fmt)
    for bad in (torch.zeros((F,) + GRID + (3,), dtype=torch.uint8),                  # the grid's shape
                torch.zeros((F + 1,) + OUT_SIZE + (3,), dtype=torch.uint8),
                torch.zeros((F,) + OUT_SIZE + (3,), dtype=torch.float32),
                torch.zeros((F, 54, 52), dtype=torch.uint8)):                        # planar-shaped under rgb24
        refused("out must be", out_size=OUT_SIZE, out=bad)
    refused("out must be", out_size=OUT_SIZE, out_format="i420", out=torch.zeros((F,) + OUT_SIZE + (3,), dtype=torch.uint8))
    assert len(seen) == 19
    # an odd delivery size is fine for rgb24
    got, _, _ = call(out_size=(35, 51))
    assert tuple(got.shape) == (F * K, 35, 51, 3)


def test_out_size_needs_an_rgb_image(ops):
    from ncahip import video
    m = _HostModel()
    m.c_out = 4
    with pytest.raises(ValueError, match="c_out"):
        video.stylize_clip(m, _frames(), step_n=1, out_dtype=torch.uint8, out_size=OUT_SIZE)
    assert m._mask_step == 0
    video.stylize_clip(m, _frames(), step_n=1, out_dtype=torch.uint8)               # without out_size a 4-channel image is served as before
    nca = _host_cond()
    nca.num_target_channels = 4
    with pytest.raises(ValueError, match="num_target_channels"):
        video.stylize_clip_conditioned(nca, _frames(), step_n=1, out_dtype=torch.uint8, out_size=OUT_SIZE, state=torch.zeros(1, nca.num_channels, *GRID))
    assert nca.calls == 0


# ------------------------------------------------------------------ 5. the symbol, and its host-side refusals (nothing is launched)
def test_symbol_declared_exported_and_bound(ops):
    from ncahip import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ncahip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == NARGS
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), SYMBOL) and len(_capi.SIGNATURES[SYMBOL]) == NARGS
    assert getattr(ops.lib(), SYMBOL).argtypes is not None


def test_c_refusals_without_a_gpu(ops):
    from ncahip import _capi
    L = ops.lib()
    P = ctypes.c_void_p
    k = (ctypes.c_int32 * 10)(*ops.rgb_yuv_coeffs("bt709", "limited"))
    N, H, W, oh, ow = 2, 10, 14, 22, 30
    need = L.ncahip_clip_resize_workspace(N, H, ow)
    assert need == N * H * ow * 3
    base = dict(src=P(0x100000), N=N, H=H, W=W, x0=0, y0=0, cw=W, ch=H, kx=P(0x200000), bx=P(0x210000), ksx=5, ky=P(0x220000), by=P(0x230000),
                ksy=5, layout=0, k=k, dst=P(0x300000), oh=oh, ow=ow, ws=P(0x400000), wsb=need, stream=None)
    order = ("src", "N", "H", "W", "x0", "y0", "cw", "ch", "kx", "bx", "ksx", "ky", "by", "ksy", "layout", "k", "dst", "oh", "ow", "ws", "wsb", "stream")
    assert len(order) == NARGS
    call = lambda **kw: getattr(L, SYMBOL)(*[{**base, **kw}[n] for n in order])      # noqa: E731
    dbytes = N * oh * ow * 3 // 2
    einval = [dict(src=None), dict(dst=None), dict(k=None), dict(layout=2), dict(layout=-1), dict(N=0), dict(oh=0), dict(ow=-2), dict(cw=0),
              dict(ksx=0), dict(wsb=need - 1),
              dict(dst=P(0x100000 + N * H * W * 3 - 1)),                             # the last byte of src
              dict(dst=P(0x100000 - dbytes + 1)),                                    # the last byte of the planar dst on the first of src
              dict(dst=P(0x400000 + need - 1)), dict(ws=P(0x100000))]
    for kw in einval:
        assert call(**kw) == _capi.EINVAL, kw
    assert b"overlap" in L.ncahip_last_error()
    erange = [dict(oh=21), dict(ow=29), dict(oh=16386), dict(ow=16386), dict(H=16385, ch=1), dict(ksx=2049), dict(ksy=2049), dict(x0=1),
              dict(y0=-1), dict(ch=H + 1), dict(kx=P(0x200001)), dict(by=P(0x230002)), dict(ky=None), dict(ws=None), dict(ws=P(0x400002))]
    for kw in erange:
        assert call(**kw) == _capi.ERANGE, kw
    # the planar dst is half as long as an RGB24 one: one byte below the overlap it passes that check (and stops at nothing else host-side
    # could refuse -- so it is not called here); the RGB24 entry point with the same pointers still refuses
    assert L.ncahip_clip_resize_u8(P(0x100000), N, H, W, 0, 0, W, H, P(0x200000), P(0x210000), 5, P(0x220000), P(0x230000), 5, P(0x100000 - dbytes), oh,
                                   ow, P(0x400000), need, None) == _capi.EINVAL
