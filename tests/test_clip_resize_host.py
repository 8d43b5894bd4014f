"""Host-side checks of the crop + resize of uint8 clip frames (no GPU): ops.clip_resize_host -- the contract of include/ncahip.h in numpy,
on the tables of the library's builder -- against the Pillow fixtures and, where Pillow is installed, against Pillow itself; the
reference's crop boxes; the tables' invariants; error paths.  Every image comparison is an equality."""
import os

import numpy as np
import pytest
import torch

FILTERS = ("bicubic", "lanczos")
# (H, W) -> (h, w): down, up, mixed, 8 : 1 (61- and 91-tap rows at 240 -> 16), tiny, one pixel in, one pixel out
SHAPES = [((37, 53), (16, 16)), ((20, 24), (40, 48)), ((33, 21), (16, 32)), ((135, 240), (16, 16)), ((5, 7), (3, 2)), ((1, 1), (4, 4)),
          ((64, 64), (1, 1))]


@pytest.fixture(scope="module")
def ops():
    from ncahip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_clip_resize.npz"))


def test_host_mirror_equals_the_pillow_fixtures(ops, golden):
    n = len(golden["case_input"])
    assert n >= 24
    for c in range(n):
        img = golden[f"in_{int(golden['case_input'][c])}"]
        assert img.shape[0] <= 45 and img.shape[1] <= 80
        box = tuple(int(v) for v in golden["case_box"][c])
        size = tuple(int(v) for v in golden["case_size"][c])
        filt = str(golden["case_filter"][c])
        got = ops.clip_resize_host(img[None], size, box, filt)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (1,) + size + (3,)
        assert np.array_equal(got[0], golden[f"out_{c}"]), (c, box, size, filt)
        got_t = ops.clip_resize_host(torch.from_numpy(img[None].copy()), size, box, filt)
        assert isinstance(got_t, torch.Tensor) and torch.equal(got_t[0], torch.from_numpy(golden[f"out_{c}"]))


def test_fixture_crops_are_the_reference_crops(golden):
    from ncahip import video
    for c in range(len(golden["case_input"])):
        kind = str(golden["case_crop"][c])
        H, W = golden[f"in_{int(golden['case_input'][c])}"].shape[:2]
        if kind in ("dynca", "conditioned"):
            assert video.reference_crop(kind, H, W) == tuple(int(v) for v in golden["case_box"][c]), (c, kind)
        elif kind == "none":
            assert tuple(int(v) for v in golden["case_box"][c]) == (0, 0, W, H)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("shape,size", SHAPES)
def test_host_mirror_equals_pillow(ops, shape, size, filt):
    Image = pytest.importorskip("PIL.Image")
    from ncahip import video
    (H, W), pil_filter = shape, {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}[filt]
    rng = np.random.default_rng(H * 1000 + W)
    frames = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    frames[1] = (frames[1] > 127) * np.uint8(255)                     # saturated: the negative lobes overshoot, both clamps act
    for crop in (None, "dynca", "conditioned"):
        box = (0, 0, W, H) if crop is None else video.reference_crop(crop, H, W)
        x0, y0, w, h = box
        want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(f[y0:y0 + h, x0:x0 + w])).resize((size[1], size[0]), pil_filter))
                         for f in frames])
        got = video.resize_frames(torch.from_numpy(frames), size, crop, filt)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2,) + size + (3,)
        assert np.array_equal(got.numpy(), want), (shape, size, filt, crop)


def test_reference_crop():
    from ncahip import video
    assert video.reference_crop("dynca", 45, 80) == (17, 0, 46, 45)            # an odd difference: one column more than rows
    assert video.reference_crop("conditioned", 45, 80) == (17, 0, 45, 45)
    assert video.reference_crop("dynca", 80, 45) == (0, 17, 45, 46)
    assert video.reference_crop("conditioned", 80, 45) == (0, 17, 45, 45)
    assert video.reference_crop("dynca", 1080, 1920) == (420, 0, 1080, 1080)
    assert video.reference_crop("conditioned", 720, 1280) == (280, 0, 720, 720)
    for kind in ("dynca", "conditioned"):
        assert video.reference_crop(kind, 32, 32) == (0, 0, 32, 32)            # square: the whole frame


@pytest.mark.parametrize("filt", FILTERS)
def test_table_invariants(ops, filt):
    support = {"bicubic": 2.0, "lanczos": 3.0}[filt]
    for n_in, n_out in [(53, 16), (24, 48), (240, 16), (7, 2), (1, 4), (64, 1), (16, 16), (1080, 256), (1920, 256), (46, 16), (45, 100)]:
        k, bounds = ops.resize_tables(n_in, n_out, filt)
        ksize = 2 * int(np.ceil(support * max(n_in / n_out, 1.0))) + 1
        assert k.dtype == np.int32 and bounds.dtype == np.int32 and k.shape == (n_out, ksize) and bounds.shape == (n_out, 2)
        assert ops.lib().ncahip_resize_ksize(n_in, n_out, {"bicubic": 0, "lanczos": 1}[filt]) == ksize
        xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
        assert (xmin >= 0).all() and (xmin + n <= n_in).all() and (n <= ksize).all() and (n >= 1).all()
        k64 = k.astype(np.int64)
        assert (255 * np.abs(k64).sum(axis=1) + (1 << 21) < (1 << 31)).all()   # int32 accumulation cannot overflow
        assert (np.abs(k64) < (1 << 23)).all()                                  # 24-bit multiplies suffice
        for i in range(n_out):
            assert not k[i, n[i]:].any()                                       # the rest of the row is zero
        assert (np.abs(k64.sum(axis=1) - (1 << 22)) <= ksize).all()            # rows sum to 1 up to one rounding per tap
        assert ops.resize_tables(n_in, n_out, filt)[0] is k                    # cached
    k, bounds = ops.resize_tables(16, 16, filt)                                # same size: the identity
    assert (bounds[:, 1] >= 1).all()
    frames = np.random.default_rng(0).integers(0, 256, (1, 16, 16, 3), dtype=np.uint8)
    assert np.array_equal(ops.clip_resize_host(frames, (16, 16), None, filt), frames)


def test_table_builder_refuses_bad_arguments(ops):
    import ctypes
    L = ops.lib()
    buf = (ctypes.c_int32 * 64)()
    assert L.ncahip_resize_ksize(0, 4, 0) == -1 and L.ncahip_resize_ksize(4, -1, 0) == -1 and L.ncahip_resize_ksize(4, 4, 2) == -1
    assert L.ncahip_resize_tables(4, 4, 0, None, buf, 5) == -1
    assert L.ncahip_resize_tables(4, 4, 0, buf, buf, 7) == -1 and b"ksize" in L.ncahip_last_error()
    assert L.ncahip_clip_resize_workspace(3, 45, 16) == 3 * 45 * 16 * 3 and L.ncahip_clip_resize_workspace(0, 45, 16) == 0


def test_errors(ops):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    u8 = torch.zeros(2, 8, 10, 3, dtype=torch.uint8)
    for fn in (ops.clip_resize_host, video.resize_frames):
        with pytest.raises(ValueError, match="resample"):
            fn(u8, (4, 4), None, "nearest")
        with pytest.raises(ValueError):
            fn(u8, (0, 4), None, "bicubic")                                    # zero sizes
        with pytest.raises(ValueError):
            fn(u8, (4, -1), None, "bicubic")
        with pytest.raises(ValueError):
            fn(u8, (4, 4), (0, 0, 0, 4), "bicubic")                            # an empty box
        for box in [(3, 0, 8, 8), (0, 1, 10, 8), (-1, 0, 4, 4), (0, 0, 11, 8)]:
            with pytest.raises(ValueError, match="outside"):
                fn(u8, (4, 4), box, "bicubic")
        with pytest.raises(ValueError):
            fn(u8[:0], (4, 4), None, "bicubic")                                # no frames
    with pytest.raises(ValueError, match="crop"):
        video.resize_frames(u8, (4, 4), "center", "bicubic")
    with pytest.raises(ValueError):
        video.resize_frames(u8.float(), (4, 4), None, "bicubic")               # 8-bit images only
    with pytest.raises(TypeError):
        ops.clip_resize_host(u8.float(), (4, 4))
    with pytest.raises(ValueError):
        ops.resize_tables(0, 4, "bicubic")
    # stylize_clip / stylize_clip_conditioned: float frames with size raise, as do an unknown crop or resample -- before anything runs
    m = DyNCA(12, 3, fc_dim=96, conditioning="edges", device=torch.device("cpu"))
    with pytest.raises(ValueError, match="uint8"):
        video.stylize_clip(m, torch.zeros(2, 3, 8, 10), step_n=1, size=(4, 4))
    with pytest.raises(ValueError, match="crop"):
        video.stylize_clip(m, u8, step_n=1, size=(4, 4), crop="middle")
    with pytest.raises(ValueError, match="resample"):
        video.stylize_clip(m, u8, step_n=1, size=(4, 4), resample="box")
    with pytest.raises(ValueError):
        video.stylize_clip(m, u8, step_n=1, size=(0, 4))
    with pytest.raises(ValueError, match="outside"):
        video.stylize_clip(m, u8, step_n=1, size=(4, 4), crop=(4, 4, 8, 8))
    from ncahip.nca import ConditionedNCA
    nca = ConditionedNCA(target_shape=(3, 4, 4), num_hidden_channels=4)
    with pytest.raises(ValueError, match="uint8"):
        video.stylize_clip_conditioned(nca, torch.zeros(2, 3, 8, 10), step_n=1, size=(4, 4))
    with pytest.raises(ValueError, match="resample"):
        video.stylize_clip_conditioned(nca, u8, step_n=1, size=(4, 4), resample="cubic")
    with pytest.raises(ValueError, match="crop"):
        video.stylize_clip_conditioned(nca, u8, step_n=1, size=(4, 4), crop="dyn")
