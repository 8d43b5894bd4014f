"""GPU tests of the crop + resize of uint8 clip frames (csrc/nca_resize.hip, ncahip_clip_resize_u8, ncahip.video.resize_frames and the
size= argument of the two clip entry points).  The kernel is held against ops.clip_resize_host (the contract in numpy, itself held
against Pillow in tests/test_clip_resize_host.py) and against the Pillow fixtures.  Every comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = ("bicubic", "lanczos")
ODD_BOX = (3, 1, 31, 29)                    # odd origin, odd size
# (H, W) -> (h, w): the host test's shapes; an output wider than one block of 64 columns; the identity; a wide output whose row length
# is no multiple of 4 (byte path of the vertical pass across several column blocks)
SHAPES = [((37, 53), (16, 16)), ((20, 24), (40, 48)), ((33, 21), (16, 32)), ((135, 240), (16, 16)), ((5, 7), (3, 2)), ((1, 1), (4, 4)),
          ((64, 64), (1, 1)), ((45, 80), (24, 100)), ((16, 16), (16, 16)), ((45, 80), (10, 67))]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        o.check_errors()                      # nothing recorded a device-side failure in this module


def _boxes(H, W):
    from ncahip import video
    boxes = [None, video.reference_crop("dynca", H, W), video.reference_crop("conditioned", H, W)]
    if ODD_BOX[0] + ODD_BOX[2] <= W and ODD_BOX[1] + ODD_BOX[3] <= H:
        boxes.append(ODD_BOX)
    return boxes


# ------------------------------------------------------------------ 1. the kernel against the host mirror
@pytest.mark.parametrize("shape,size", SHAPES)
def test_clip_resize_equals_the_host_mirror(ops, shape, size):
    H, W = shape
    gen = torch.Generator().manual_seed(H * 1000 + W)
    frames = torch.randint(0, 256, (3, H, W, 3), generator=gen, dtype=torch.uint8)
    frames[1] = (frames[1] > 127).to(torch.uint8) * 255             # saturated: both clamps act
    dev = frames.to(DEV)
    n_box = 0
    for box in _boxes(H, W):
        for filt in FILTERS:
            want = ops.clip_resize_host(frames, size, box, filt)
            for N in (1, 3):
                got = ops.clip_resize(dev[:N], size, box, filt)
                assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (N,) + size + (3,)
                assert torch.equal(got.cpu(), want[:N]), (shape, size, box, filt, N)
            if box is None and shape == size:
                assert torch.equal(got.cpu(), frames)               # same size, no crop: a copy
        n_box += 1
    assert n_box >= 3
    ops.check_errors()


def test_resize_frames_routes_by_device(ops):
    from ncahip import video
    frames = torch.randint(0, 256, (2, 45, 80, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    for crop, filt in (("dynca", "bicubic"), ("conditioned", "lanczos"), (None, "lanczos"), (ODD_BOX, "bicubic")):
        host = video.resize_frames(frames, (16, 24), crop, filt)
        dev = video.resize_frames(frames.to(DEV), (16, 24), crop, filt)
        assert not host.is_cuda and dev.is_cuda and torch.equal(dev.cpu(), host)
    ops.check_errors()


# ------------------------------------------------------------------ 2. the Pillow fixtures
def test_clip_resize_equals_the_pillow_fixtures(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "g12_clip_resize.npz"))
    for c in range(len(g["case_input"])):
        img = torch.from_numpy(g[f"in_{int(g['case_input'][c])}"])[None].to(DEV)
        box = tuple(int(v) for v in g["case_box"][c])
        size = tuple(int(v) for v in g["case_size"][c])
        got = ops.clip_resize(img, size, box, str(g["case_filter"][c]))
        assert torch.equal(got[0].cpu(), torch.from_numpy(g[f"out_{c}"])), (c, box, size, str(g["case_filter"][c]))
    ops.check_errors()


# ------------------------------------------------------------------ 3. byte phases
@pytest.mark.parametrize("filt", FILTERS)
def test_clip_resize_unaligned_uint8_views(ops, filt):
    """Frames whose data pointer is odd and whose rows start at every byte phase (W * 3 = 201): the aligned dword loads of the
    horizontal pass must pick the same pixels, the dwords that straddle the tensor's two ends included."""
    N, H, W = 2, 19, 67
    buf = torch.randint(0, 256, (N * H * W * 3 + 1,), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).to(DEV)
    frames = buf[1:].view(N, H, W, 3)
    assert frames.data_ptr() % 4 != 0 and frames.is_contiguous() and (W * 3) % 4 != 0
    for box in (None, (0, 0, 67, 19), (1, 0, 66, 19), (5, 3, 62, 16), (2, 18, 65, 1)):      # first and last byte of the tensor included
        for size in ((8, 16), (19, 67), (5, 70)):
            got = ops.clip_resize(frames, size, box, filt)
            assert torch.equal(got.cpu(), ops.clip_resize_host(frames.cpu(), size, box, filt)), (box, size)
    ops.check_errors()


# ------------------------------------------------------------------ 4. saturation
@pytest.mark.parametrize("filt", FILTERS)
def test_clip_resize_saturation(ops, filt):
    for value in (0, 255):
        flat = torch.full((2, 37, 53, 3), value, dtype=torch.uint8, device=DEV)
        for size in ((16, 16), (50, 70)):
            out = ops.clip_resize(flat, size, None, filt)
            assert int(out.min()) == value and int(out.max()) == value, (value, size)
    yy, xx = torch.meshgrid(torch.arange(24), torch.arange(40), indexing="ij")
    checker = (((yy + xx) % 2) * 255).to(torch.uint8)[None, :, :, None].expand(2, 24, 40, 3).contiguous()
    seen = set()
    for size in ((17, 29), (36, 60), (24, 40), (31, 13)):
        got = ops.clip_resize(checker.to(DEV), size, None, filt).cpu()
        assert torch.equal(got, ops.clip_resize_host(checker, size, None, filt)), size
        seen |= {int(got.min()), int(got.max())}
    assert seen >= {0, 255}                                          # the clamp on the filters' negative lobes acted at both ends
    ops.check_errors()


# ------------------------------------------------------------------ 5. end to end
def _dynca():
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _dynca_extra():
    from ncahip.models.dynca_extra import DyNCA
    torch.manual_seed(0)
    m = DyNCA(13, 3, fc_dim=96, padding_mode="circular", pos_emb="CPE", perception_scales=[0], device=torch.device(DEV))
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


def _decoder_frames():
    return torch.randint(0, 256, (3, 37, 53, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)      # host, decoder-native


@pytest.mark.parametrize("rng", ["torch", "philox"])
@pytest.mark.parametrize("make", [_dynca, _dynca_extra])
def test_stylize_clip_size_equals_resizing_beforehand(ops, make, rng):
    from ncahip import video
    m, frames, size = make(), _decoder_frames(), (16, 16)
    m.mask_rng, m.mask_seed = rng, 11
    small = video.resize_frames(frames.to(DEV), size, "dynca", "bicubic")
    assert tuple(small.shape) == (3, 16, 16, 3)

    def run(fr, **kw):
        torch.manual_seed(7)                     # the fire-mask source, both kinds, back to the same point
        m._mask_step = 40
        imgs, h = video.stylize_clip(m, fr, step_n=2, out_dtype=torch.uint8, **kw)
        assert video.stylize_clip.last_path == "clip"
        return imgs.clone(), h.clone()

    want, want_h = run(small)
    assert tuple(want.shape) == (3, 16, 16, 3) and want_h.shape[2:] == (16, 16)
    for kw in ({}, {"frames_per_call": 1}, {"frames_per_call": 32}):
        for fr in (frames, frames.to(DEV)):
            got, got_h = run(fr, size=size, **kw)
            assert torch.equal(got, want) and torch.equal(got_h, want_h), kw
    # the defaults are the reference's path for this family: a different crop or filter gives different frames
    other, _ = run(frames, size=size, crop="conditioned", resample="lanczos")
    assert not torch.equal(other, want)
    # float32 images and the continuation of a state, which has the model grid's shape
    a, ha = run(frames[:2], size=size)
    b, hb = video.stylize_clip(m, frames[2:], step_n=2, out_dtype=torch.uint8, size=size, state=ha)
    assert torch.equal(torch.cat([a, b]), want) and torch.equal(hb, want_h)
    torch.manual_seed(7)
    m._mask_step = 40
    f32, _ = video.stylize_clip(m, frames, step_n=2, size=size)
    assert tuple(f32.shape) == (3, 3, 16, 16) and f32.dtype == torch.float32
    ops.check_errors()


def test_stylize_clip_size_on_the_loop_route(ops):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="pos_emb", edge_transform="tanh", perception_scales=[0], device=torch.device(DEV))
    frames, size = _decoder_frames(), (16, 16)
    m.mask_rng, m.mask_seed = "philox", 3
    small = video.resize_frames(frames.to(DEV), size, "dynca", "bicubic")
    m._mask_step = 0
    want, want_h = video.stylize_clip(m, small, step_n=2, out_dtype=torch.uint8)
    assert video.stylize_clip.last_path == "loop"
    m._mask_step = 0
    got, got_h = video.stylize_clip(m, frames, step_n=2, out_dtype=torch.uint8, size=size)
    assert video.stylize_clip.last_path == "loop" and torch.equal(got, want) and torch.equal(got_h, want_h)
    ops.check_errors()


@pytest.mark.parametrize("rng", ["torch", "philox"])
def test_stylize_clip_conditioned_size_equals_resizing_beforehand(ops, rng):
    from ncahip import video
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(0)
    m = ConditionedNCA(target_shape=(3, 16, 16)).to(DEV)            # the default model
    m.mask_rng, m.mask_seed = rng, 11
    frames, size = _decoder_frames(), (16, 16)
    small = video.resize_frames(frames.to(DEV), size, "conditioned", "lanczos")

    def run(fr, **kw):
        torch.manual_seed(7)
        m._mask_step = 40
        imgs, h = video.stylize_clip_conditioned(m, fr, step_n=2, out_dtype=torch.uint8, **kw)
        assert video.stylize_clip_conditioned.last_path == "clip"
        return imgs.clone(), h.clone()

    want, want_h = run(small)
    assert tuple(want.shape) == (3, 16, 16, 3) and tuple(want_h.shape[2:]) == (16, 16)
    for kw in ({}, {"frames_per_call": 1}, {"frames_per_call": 32}):
        got, got_h = run(frames, size=size, **kw)
        assert torch.equal(got, want) and torch.equal(got_h, want_h), kw
    # a state of the model grid's shape continues; one of the frames' shape is refused
    run(frames, size=size, state=want_h)
    with pytest.raises(ValueError, match="state"):
        video.stylize_clip_conditioned(m, frames, step_n=2, size=size, state=torch.zeros(1, m.num_channels, 37, 53, device=DEV))
    with pytest.raises(ValueError, match="uint8"):
        video.stylize_clip_conditioned(m, torch.rand(3, 3, 37, 53), step_n=2, size=size)
    ops.check_errors()


# ------------------------------------------------------------------ 6. what the entry point refuses
def _raw(ops, frames, box, kx, bx, ksx, ky, by, ksy, out, ws, ws_bytes):
    from ncahip import _capi
    N, H, W, _ = frames.shape
    _, out_h, out_w, _ = out.shape
    ptr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()      # noqa: E731
    _capi.check(ops.lib().ncahip_clip_resize_u8(ptr(frames), N, H, W, *box, ptr(kx), ptr(bx), ksx, ptr(ky), ptr(by), ksy, ptr(out), out_h, out_w,
                                                ptr(ws), ws_bytes, ops._stream()), "clip_resize")


def test_clip_resize_refusals(ops):
    from ncahip._capi import NcaHipError
    erange = "rc=-2"
    # a dimension above 16384, in and out
    with pytest.raises(NcaHipError, match=erange):
        ops.clip_resize(torch.zeros(1, 1, 16385, 3, dtype=torch.uint8, device=DEV), (1, 8192))
    with pytest.raises(NcaHipError, match=erange):
        ops.clip_resize(torch.zeros(1, 16385, 1, 3, dtype=torch.uint8, device=DEV), (8192, 1))
    with pytest.raises(NcaHipError, match=erange):
        ops.clip_resize(torch.zeros(1, 2, 2, 3, dtype=torch.uint8, device=DEV), (1, 16385))
    with pytest.raises(NcaHipError, match=erange):
        ops.clip_resize(torch.zeros(1, 2, 2, 3, dtype=torch.uint8, device=DEV), (16385, 1))
    # a table row wider than 2048: 16384 -> 4 is a 4096 : 1 shrink
    for filt in FILTERS:
        with pytest.raises(NcaHipError, match=erange):
            ops.clip_resize(torch.zeros(1, 1, 16384, 3, dtype=torch.uint8, device=DEV), (1, 4), None, filt)
    # below the Python layer: crops outside the frame, null and misaligned tables and workspace
    frames = torch.randint(0, 256, (2, 20, 24, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    out = torch.empty(2, 8, 12, 3, dtype=torch.uint8, device=DEV)
    dev = torch.device(DEV, torch.cuda.current_device())
    (kx, bx), (ky, by) = ops._resize_tables_dev(24, 12, "bicubic", dev), ops._resize_tables_dev(20, 8, "bicubic", dev)
    ksx, ksy = kx.shape[1], ky.shape[1]
    need = ops.lib().ncahip_clip_resize_workspace(2, 20, 12)
    assert need == 2 * 20 * 12 * 3
    ws = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    good = dict(frames=frames, box=(0, 0, 24, 20), kx=kx, bx=bx, ksx=ksx, ky=ky, by=by, ksy=ksy, out=out, ws=ws, ws_bytes=need)
    _raw(ops, **good)
    assert torch.equal(out.cpu(), ops.clip_resize_host(frames.cpu(), (8, 12), None, "bicubic"))
    for box in [(1, 0, 24, 20), (0, 1, 24, 20), (-1, 0, 24, 20), (0, -1, 24, 20), (0, 0, 25, 20), (0, 0, 24, 21), (2 ** 31 - 1, 0, 24, 20)]:
        with pytest.raises(NcaHipError, match=erange):
            _raw(ops, **{**good, "box": box})
    odd = lambda t: t.data_ptr() + 1                                 # noqa: E731
    for name in ("kx", "bx", "ky", "by"):
        with pytest.raises(NcaHipError, match=erange):
            _raw(ops, **{**good, name: None})
        with pytest.raises(NcaHipError, match=erange):
            _raw(ops, **{**good, name: odd(good[name])})
    with pytest.raises(NcaHipError, match=erange):
        _raw(ops, **{**good, "ws": None})
    for off in (1, 2, 3):
        with pytest.raises(NcaHipError, match=erange):
            _raw(ops, **{**good, "ws": ws.data_ptr() + off})
    # argument errors of the other kind: a short workspace, null frames, overlapping buffers
    with pytest.raises(NcaHipError, match="rc=-1"):
        _raw(ops, **{**good, "ws_bytes": need - 1})
    with pytest.raises(NcaHipError, match="rc=-1"):
        _raw(ops, **{**good, "frames": frames, "out": frames[:, :8, :12]})
    ops.check_errors()
    # nothing above launched anything that wrote: the good call's result is still there
    assert torch.equal(out.cpu(), ops.clip_resize_host(frames.cpu(), (8, 12), None, "bicubic"))
