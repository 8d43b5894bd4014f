"""GPU tests of images at delivery size (the planar vertical pass of csrc/nca_resize.hip, ncahip_clip_resize_u8_yuv420,
video.resize_frames(out_format=...) and out_size= / out_resample= of the two clip entry points).  The kernel is held against
ops.clip_resize_to_yuv420_host (the composition of the two mirrors, held against Pillow in tests/test_clip_out_size_host.py), against the
Pillow fixture g13_clip_upscale.npz and against clip_resize followed by rgb_to_yuv420 on the device; the clip calls against
resize_frames of the images of the same call without out_size.  Every comparison is torch.equal."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = ("bicubic", "lanczos")
FORMATS = ("i420", "nv12")
MODES = [("bt601", "limited"), ("bt601", "full"), ("bt709", "limited"), ("bt709", "full")]
# (H, W) -> (out_h, out_w): non-integer ratios with out_w % 4 == 2; the host tests' sizes; an odd grid at exactly 2 x; the identity;
# shrinking through the same pass; a 6 x 6 planar image (V plane at byte 45, the next image at byte 54)
SIZES = [((10, 14), (22, 30)), ((16, 24), (36, 52)), ((9, 7), (18, 14)), ((20, 24), (20, 24)), ((45, 80), (24, 44)), ((4, 6), (6, 6))]
ALL_MODES_AT = ((10, 14), (22, 30))
GUARD, FILL = 16, 0xA5
GRID, OUT_SIZE, F, K, STEP_N, PER_CALL = (16, 32), (36, 68), 5, 2, 2, 2


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        o.check_errors()                      # nothing recorded a device-side failure in this module


def _frames(N, H, W, seed):
    """Random frames (host); frame 1 saturated: both clamps of the passes act, and the limited range's ends."""
    f = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    if N > 1:
        f[1] = (f[1] > 127).to(torch.uint8) * 255
    return f


def _checker(N, H, W):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    c = (((yy + xx) % 2) * 255).to(torch.uint8)[None, :, :, None].expand(N, H, W, 3).contiguous()
    c[..., 1] = 255 - c[..., 1]                                       # coloured: chroma away from 128
    return c


def _raw(ops, frames, box, size, filt, fmt, mode, dst, ws="new", ws_bytes=None, **over):
    """The C entry point on tensors as they are (any view; an int is an address, None a null pointer): returns its return code."""
    from ncahip import _capi
    N, H, W, _ = frames.shape
    x0, y0, cw, ch = box if box is not None else (0, 0, W, H)
    dev = torch.device(DEV, torch.cuda.current_device())
    (kx, bx), (ky, by) = ops._resize_tables_dev(cw, size[1], filt, dev), ops._resize_tables_dev(ch, size[0], filt, dev)
    need = ops.lib().ncahip_clip_resize_workspace(N, ch, size[1])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if isinstance(ws, str) else ws
    k = ops.rgb_yuv_coeffs(*mode)
    a = dict(src=frames.data_ptr(), N=N, H=H, W=W, x0=x0, y0=y0, cw=cw, ch=ch, kx=kx.data_ptr(), bx=bx.data_ptr(), ksx=kx.shape[1], ky=ky.data_ptr(),
             by=by.data_ptr(), ksy=ky.shape[1], layout=_capi.YUV_LAYOUTS[fmt], k=k.ctypes.data, dst=dst if isinstance(dst, int) or dst is None else dst.data_ptr(),
             oh=size[0], ow=size[1], ws=ws if isinstance(ws, int) or ws is None else ws.data_ptr(), wsb=need if ws_bytes is None else ws_bytes)
    a.update(over)
    P = lambda v: None if v is None else ctypes.c_void_p(v)          # noqa: E731
    return ops.lib().ncahip_clip_resize_u8_yuv420(P(a["src"]), a["N"], a["H"], a["W"], a["x0"], a["y0"], a["cw"], a["ch"], P(a["kx"]), P(a["bx"]), a["ksx"],
                                                  P(a["ky"]), P(a["by"]), a["ksy"], a["layout"], P(a["k"]), P(a["dst"]), a["oh"], a["ow"], P(a["ws"]),
                                                  a["wsb"], ops._stream())


# ------------------------------------------------------------------ 1. the kernel against the host mirror and the device composition
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape,size", SIZES)
def test_kernel_equals_the_host_mirror(ops, shape, size, fmt):
    H, W = shape
    frames = _frames(3, H, W, 1000 * H + W)
    dev = frames.to(DEV)
    modes = MODES if (shape, size) == ALL_MODES_AT else [("bt709", "limited")]
    for filt in FILTERS:
        rgb = ops.clip_resize(dev, size, None, filt)
        for mode in modes:
            want = ops.clip_resize_to_yuv420_host(frames, size, None, filt, fmt, *mode)
            for N in (1, 3):
                got = ops.clip_resize_to_yuv420(dev[:N], size, None, filt, fmt, *mode)
                assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (N, 3 * size[0] // 2, size[1])
                assert torch.equal(got.cpu(), want[:N]), (shape, size, filt, mode, N)
            assert torch.equal(got, ops.rgb_to_yuv420(rgb, fmt, *mode))                   # the two launches and the conversion launch
        if shape == size:                                                               # identity tables: the conversion of the frames
            assert torch.equal(got, ops.rgb_to_yuv420(dev, fmt, *modes[-1]))
    ops.check_errors()


@pytest.mark.parametrize("fmt", FORMATS)
def test_kernel_equals_the_pillow_fixture(ops, golden_dir, fmt):
    g = np.load(os.path.join(golden_dir, "g13_clip_upscale.npz"))
    assert len(g["case_input"]) >= 8
    for c in range(len(g["case_input"])):
        img = torch.from_numpy(g[f"in_{int(g['case_input'][c])}"])[None]
        size, filt = tuple(int(v) for v in g["case_size"][c]), str(g["case_filter"][c])
        pillow = torch.from_numpy(g[f"out_{c}"])[None]
        assert torch.equal(ops.clip_resize(img.to(DEV), size, None, filt).cpu(), pillow), c       # the RGB path enlarges as Pillow does
        got = ops.clip_resize_to_yuv420(img.to(DEV), size, None, filt, fmt, "bt601", "full")
        assert torch.equal(got.cpu(), ops.rgb_to_yuv420_host(pillow, fmt, "bt601", "full")), (c, size, filt)
    ops.check_errors()


@pytest.mark.parametrize("filt", FILTERS)
def test_checkerboard_is_clamped_before_the_yuv_arithmetic(ops, filt):
    checker = _checker(3, 16, 24)
    seen = set()
    for size in ((36, 52), (22, 30), (16, 24), (12, 14)):
        rgb = ops.clip_resize(checker.to(DEV), size, None, filt)
        seen |= {int(rgb.min()), int(rgb.max())}
        for fmt in FORMATS:
            got = ops.clip_resize_to_yuv420(checker.to(DEV), size, None, filt, fmt, "bt709", "full")
            assert torch.equal(got.cpu(), ops.clip_resize_to_yuv420_host(checker, size, None, filt, fmt, "bt709", "full")), (size, fmt)
    assert seen >= {0, 255}                                          # the filters' lobes reached both clamps
    for value in (0, 255):
        flat = torch.full((2, 16, 24, 3), value, dtype=torch.uint8, device=DEV)
        got = ops.clip_resize_to_yuv420(flat, (36, 52), None, filt, "i420", "bt709", "full")
        assert int(got[:, :36].min()) == value == int(got[:, :36].max()) and int(got[:, 36:].min()) == 128 == int(got[:, 36:].max())
    ops.check_errors()


@pytest.mark.parametrize("fmt", FORMATS)
def test_views_one_byte_off_alignment_and_guards(ops, fmt):
    """src and dst at every byte offset of an aligned storage (src through the horizontal pass's loader, dst through the block writer's
    dword / half / byte stores); nothing is written outside dst."""
    mode = ("bt601", "limited")
    for (H, W), size in (((10, 14), (22, 30)), ((4, 6), (6, 6)), ((16, 24), (36, 52))):
        frames = _frames(3, H, W, 77 + H)
        nbytes = 3 * 3 * size[0] * size[1] // 2
        for filt in FILTERS:
            want = ops.clip_resize_to_yuv420_host(frames, size, None, filt, fmt, *mode).to(DEV)
            for off in range(4):
                sbuf = torch.empty(frames.numel() + 4, dtype=torch.uint8, device=DEV)
                src = sbuf[off:off + frames.numel()].view(frames.shape)
                src.copy_(frames)
                dbuf = torch.full((GUARD + 3 + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
                dst = dbuf[GUARD + off:GUARD + off + nbytes]
                assert src.data_ptr() % 4 == off and dst.data_ptr() % 4 == off
                assert _raw(ops, src, None, size, filt, fmt, mode, dst) == 0, ops.lib().ncahip_last_error()
                assert torch.equal(dst.view(3, 3 * size[0] // 2, size[1]), want), (size, filt, off)
                assert bool((dbuf[:GUARD + off] == FILL).all()) and bool((dbuf[GUARD + off + nbytes:] == FILL).all()), (size, filt, off)
    ops.check_errors()


def test_crop_box(ops):
    frames = _frames(3, 45, 80, 5)
    for box in ((3, 1, 31, 29), (0, 0, 80, 45), (79, 44, 1, 1), (2, 18, 65, 9)):
        for size in ((22, 30), (40, 36)):
            for fmt, filt in (("i420", "bicubic"), ("nv12", "lanczos")):
                got = ops.clip_resize_to_yuv420(frames.to(DEV), size, box, filt, fmt)
                assert torch.equal(got.cpu(), ops.clip_resize_to_yuv420_host(frames, size, box, filt, fmt)), (box, size, fmt)
    ops.check_errors()


def test_resize_frames_out_format_routes_by_device(ops):
    from ncahip import video
    frames = _frames(2, 20, 24, 9)
    for fmt in FORMATS:
        kw = dict(out_format=fmt, out_yuv_matrix="bt601", out_yuv_range="full")
        host = video.resize_frames(frames, (30, 44), "dynca", "lanczos", **kw)
        dev = video.resize_frames(frames.to(DEV), (30, 44), "dynca", "lanczos", **kw)
        assert not host.is_cuda and dev.is_cuda and torch.equal(dev.cpu(), host)
    planar = video.rgb_to_yuv420(frames.to(DEV), "nv12")
    got = video.resize_frames(planar, (30, 44), None, "bicubic", pixel_format="nv12", out_format="i420")
    assert torch.equal(got, video.rgb_to_yuv420(video.resize_frames(planar, (30, 44), None, "bicubic", pixel_format="nv12"), "i420"))
    ops.check_errors()


# ------------------------------------------------------------------ 2. what the entry point refuses
def test_c_refusals(ops):
    from ncahip import _capi
    frames = _frames(2, 10, 14, 2).to(DEV)
    size, filt, fmt, mode = (22, 30), "bicubic", "i420", ("bt709", "limited")
    dst = torch.full((2, 33, 30), FILL, dtype=torch.uint8, device=DEV)
    need = ops.lib().ncahip_clip_resize_workspace(2, 10, 30)
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    good = dict(frames=frames, box=None, size=size, filt=filt, fmt=fmt, mode=mode, dst=dst, ws=ws)
    assert _raw(ops, **good) == 0
    want = ops.clip_resize_to_yuv420_host(frames.cpu(), size, None, filt, fmt, *mode)
    assert torch.equal(dst.cpu(), want)
    for over in (dict(src=None), dict(dst=None), dict(k=None), dict(layout=2), dict(layout=-1), dict(N=0), dict(oh=0), dict(ow=-2), dict(wsb=need - 1),
                 dict(dst=frames.data_ptr()), dict(dst=ws.data_ptr()), dict(ws=frames.data_ptr() & ~3)):
        assert _raw(ops, **{**good, **over}) == _capi.EINVAL, over
    for over in (dict(oh=21), dict(ow=29), dict(oh=16386), dict(ow=16386), dict(ksx=2049), dict(ksy=2049), dict(x0=1), dict(y0=-1), dict(cw=15),
                 dict(ch=11), dict(kx=None), dict(by=None), dict(ws=None), dict(ws=ws.data_ptr() + 1), dict(ws=ws.data_ptr() + 2)):
        assert _raw(ops, **{**good, **over}) == _capi.ERANGE, over
    for name in ("kx", "bx", "ky", "by"):
        dev = torch.device(DEV, torch.cuda.current_device())
        t = dict(zip(("kx", "bx"), ops._resize_tables_dev(14, 30, filt, dev)), **dict(zip(("ky", "by"), ops._resize_tables_dev(10, 22, filt, dev))))
        assert _raw(ops, **{**good, name: t[name].data_ptr() + 2}) == _capi.ERANGE, name
    with pytest.raises(ValueError, match="even"):
        ops.clip_resize_to_yuv420(frames, (21, 30))
    with pytest.raises(ValueError, match="out must be"):
        ops.clip_resize_to_yuv420(frames, size, out=torch.empty(2, 22, 30, 3, dtype=torch.uint8, device=DEV))
    ops.check_errors()
    assert torch.equal(dst.cpu(), want)                              # nothing above launched anything that wrote


# ------------------------------------------------------------------ 3. the clip calls
def _dynca(scales=(0,), conditioning="edges"):
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning=conditioning, edge_transform="tanh", perception_scales=list(scales),
              device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _dynca_two_scale():
    return _dynca((0, 1))


def _dynca_loop():
    return _dynca((0, 1, 2))


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


def _conditioned_bf16():
    return _conditioned()


def _runner(make, grid=GRID):
    """run(frames, **kw) -> (images, state, _mask_step after) of the model's clip entry point from the same fire-mask position and state."""
    from ncahip import video
    m = make()
    m.mask_rng, m.mask_seed = "philox", 11
    cond = make in (_conditioned, _conditioned_bf16)
    fn = video.stylize_clip_conditioned if cond else video.stylize_clip
    route = "loop" if make is _dynca_loop else "clip"
    base = {}
    if cond:                                                         # a non-square grid: the state is passed
        x0 = torch.rand(1, m.num_channels, *grid, generator=torch.Generator().manual_seed(4)).to(DEV)
        x0[:, 3] = 1.0
        base = {"state": x0, **({"precision": "bf16"} if make is _conditioned_bf16 else {})}

    def run(frames, **kw):
        m._mask_step = 40
        imgs, h = fn(m, frames, **{**dict(step_n=STEP_N, steps_per_frame=K, out_dtype=torch.uint8, frames_per_call=PER_CALL), **base, **kw})
        assert fn.last_path == route
        return imgs, h.clone(), m._mask_step

    return run, fn, m


ROUTES = [_dynca, _dynca_two_scale, _dynca_extra, _dynca_loop, _conditioned, _conditioned_bf16]


@pytest.mark.parametrize("make", ROUTES)
def test_clip_calls_deliver_the_resize_of_their_grid_images(ops, make):
    from ncahip import video
    run, fn, _ = _runner(make)
    frames = _frames(F, *GRID, 7).to(DEV)
    plain, want_h, want_step = run(frames)
    assert tuple(plain.shape) == (F * K,) + GRID + (3,) and fn.last_download is None and len(torch.unique(plain)) > 20
    cases = [("rgb24", "bicubic", {}), ("i420", "bicubic", {}), ("i420", "lanczos", dict(out_yuv_matrix="bt601", out_yuv_range="full"))]
    if make is _dynca:
        cases.append(("nv12", "bicubic", {}))
    for fmt, resample, ykw in cases:
        want = video.resize_frames(plain, OUT_SIZE, None, resample, out_format="rgb24")
        shape = OUT_SIZE + (3,)
        if fmt != "rgb24":
            want, shape = video.rgb_to_yuv420(want, fmt, *(ykw.get("out_yuv_matrix", "bt709"), ykw.get("out_yuv_range", "limited"))), (54, 68)
        kw = dict(out_size=OUT_SIZE, out_resample=resample, out_format=fmt, **ykw)
        for per_call in (1, 5):
            got, h, step = run(frames, frames_per_call=per_call, **kw)
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (F * K,) + shape and fn.last_download is None
            assert torch.equal(got, want) and torch.equal(h, want_h) and step == want_step, (fmt, resample, per_call)
        if resample == "bicubic":
            host = want.cpu()
            out = torch.full((F * K,) + shape, FILL, dtype=torch.uint8).pin_memory()
            got, h, step = run(frames, out=out, **kw)                                 # valid at return: no synchronize before the compare
            assert got is out and fn.last_download == "overlapped" and torch.equal(out, host) and torch.equal(h, want_h) and step == want_step
            out = torch.full((F * K,) + shape, FILL, dtype=torch.uint8)
            got, h, _ = run(frames, out=out, **kw)
            assert got is out and fn.last_download == "sync" and torch.equal(out, host) and torch.equal(h, want_h)
    ops.check_errors()


def test_pinned_frames_and_pinned_out_together(ops):
    """Host frames in pinned memory and a pinned out: both side streams at work; last_upload / last_download mean what they mean."""
    from ncahip import video
    run, fn, _ = _runner(_dynca)
    frames = _frames(F, *GRID, 8)
    plain, want_h, _ = run(frames.to(DEV))
    want = video.rgb_to_yuv420(video.resize_frames(plain, OUT_SIZE), "i420").cpu()
    out = torch.full((F * K, 54, 68), FILL, dtype=torch.uint8).pin_memory()
    got, h, _ = run(frames.pin_memory(), out=out, out_size=OUT_SIZE, out_format="i420")
    assert got is out and fn.last_upload == "overlapped" and fn.last_download == "overlapped" and torch.equal(out, want) and torch.equal(h, want_h)
    run(frames.to(DEV), out_size=OUT_SIZE)
    assert fn.last_upload == "sync" and fn.last_download is None
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_odd_grid_with_an_even_out_size(ops, make):
    from ncahip import video
    grid = (15, 32)
    run, fn, _ = _runner(make, grid)
    frames = _frames(3, *grid, 9).to(DEV)
    plain, want_h, _ = run(frames)
    got, h, _ = run(frames, out_size=OUT_SIZE, out_format="i420")
    assert torch.equal(got, video.rgb_to_yuv420(video.resize_frames(plain, OUT_SIZE), "i420")) and torch.equal(h, want_h)
    with pytest.raises(ValueError, match="even"):
        run(frames, out_format="i420")                               # without out_size the rule is the grid's
    with pytest.raises(ValueError, match="even"):
        run(frames, out_size=(35, 68), out_format="i420")
    ops.check_errors()


@pytest.mark.parametrize("make", [_dynca, _conditioned])
def test_refusals_leave_the_model_where_it_was(ops, make):
    run, fn, m = _runner(make)
    frames = _frames(3, *GRID, 6).to(DEV)
    gen_state = torch.cuda.get_rng_state()
    bad_calls = [dict(out_size=OUT_SIZE, out_dtype=torch.float32), dict(out_size=(36,)), dict(out_size=(0, 68)), dict(out_size=OUT_SIZE, out_resample="cubic"),
                 dict(out_size=(35, 68), out_format="nv12"), dict(out_size=OUT_SIZE, out=torch.empty((3 * K,) + GRID + (3,), dtype=torch.uint8, device=DEV)),
                 dict(out_size=OUT_SIZE, out_format="i420", out=torch.empty((3 * K,) + OUT_SIZE + (3,), dtype=torch.uint8).pin_memory())]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            run(frames, **kw)
        assert m._mask_step == 40 and torch.equal(torch.cuda.get_rng_state(), gen_state), kw
    ops.check_errors()
