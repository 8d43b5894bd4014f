"""Host-side checks of the fused sliced-Wasserstein loss (no GPU): the five entry points are declared, exported and in the ctypes
table, the workspace size is host arithmetic, argument validation answers before any launch, the `slw_impl` switch of
ncahip.loss.Loss knows both values and refuses an unknown one, and the nearest-resample index map is F.interpolate's."""
import ctypes
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_capi_exports import header_prototypes

SLW_SYMBOLS = {"ncahip_slw_workspace": 4, "ncahip_slw_project_f32": 10, "ncahip_slw_sort_f32": 5, "ncahip_slw_loss_fwd_f32": 10,
               "ncahip_slw_bwd_f32": 14}


def test_symbols_declared_exported_and_bound():
    from ncahip import _capi
    protos = header_prototypes()
    L = _capi.lib()
    for name, nargs in SLW_SYMBOLS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert hasattr(L, name), name
        assert len(_capi.SIGNATURES[name]) == nargs, name
    assert _capi.version() == 300


def test_workspace_is_host_arithmetic():
    from ncahip import _capi
    L = _capi.lib()
    # the larger of the backward's dk [B, 32, n] and the forward's partials (one per row and 4096 positions, one per sample); floats
    assert L.ncahip_slw_workspace(32, 512, 65536, 65536) == 32 * 32 * 65536 * 4
    assert L.ncahip_slw_workspace(2, 64, 1000, 1536) == 2 * 32 * 1000 * 4
    assert L.ncahip_slw_workspace(3, 3, 37, 50) == 3 * 32 * 37 * 4
    assert L.ncahip_slw_workspace(1, 8, 1, 1) == (32 + 1) * 4              # n = 1: 32 partials + 1 sample sum outweigh 32 dk entries
    assert L.ncahip_slw_workspace(1, 4, 20000, 12345) == 32 * 20000 * 4
    for bad in ((0, 64, 16, 16), (1025, 64, 16, 16), (2, 0, 16, 16), (2, 5, 16, 16), (2, 6, 16, 16), (2, 516, 16, 16), (2, 64, 0, 16),
                (2, 64, 65537, 16), (2, 64, 16, 0), (2, 64, 16, 65537), (-1, 64, 16, 16)):
        assert L.ncahip_slw_workspace(*bad) == 0, bad
    assert L.ncahip_ot_moment_workspace(32, 1000, 512) == 32 * (512 + 8 + 36) * 4     # the OT workspaces are what they were
    assert L.ncahip_ot_workspace(32, 1000, 512) == 2 * 16 * 32 * 1000 * 8


def test_argument_validation_without_gpu():
    from ncahip import _capi
    L = _capi.lib()
    a, b, c, d, e, f, g, h = (ctypes.c_void_p(0x1000 * k) for k in range(1, 9))   # never dereferenced: every call below is refused
    big = 1 << 40

    def project(B=2, ch=64, n=1000, m=1536, source=a, target=b, proj=c, ks=d, kt=e):
        return L.ncahip_slw_project_f32(source, target, proj, ks, kt, B, ch, n, m, None)

    def sort(rows=64, n=1000, keys=a, perm=b):
        return L.ncahip_slw_sort_f32(keys, perm, rows, n, None)

    def fwd(B=2, n=1000, m=1536, s=a, t=b, jmap=c, loss=d, ws=e, nbytes=big):
        return L.ncahip_slw_loss_fwd_f32(s, t, jmap, loss, B, n, m, ws, nbytes, None)

    def bwd(B=2, ch=64, n=1000, m=1536, s=a, t=b, jmap=c, perm=d, proj=e, g_loss=f, dsource=g, ws=h, nbytes=big):
        return L.ncahip_slw_bwd_f32(s, t, jmap, perm, proj, g_loss, dsource, B, ch, n, m, ws, nbytes, None)

    for call in (project, fwd, bwd):
        assert call(n=0) == -2 and b"n=0" in L.ncahip_last_error(), call.__name__
        assert call(n=65537) == -2 and b"n=65537" in L.ncahip_last_error(), call.__name__
        assert call(m=0) == -2 and b"m=0" in L.ncahip_last_error(), call.__name__
        assert call(m=65537) == -2 and b"m=65537" in L.ncahip_last_error(), call.__name__
        assert call(B=1025) == -2 and b"B=1025" in L.ncahip_last_error(), call.__name__
        assert call(B=0) == -1 and b"B=0" in L.ncahip_last_error(), call.__name__
    for call in (project, bwd):
        for ch in (5, 6, 2, 516, 0):
            assert call(ch=ch) == -2 and f"c={ch}".encode() in L.ncahip_last_error(), (call.__name__, ch)
    assert sort(n=0) == -2 and b"n=0" in L.ncahip_last_error()
    assert sort(n=65537) == -2 and b"n=65537" in L.ncahip_last_error()
    assert sort(rows=65536) == -2 and b"rows=65536" in L.ncahip_last_error()
    assert sort(rows=0) == -1 and b"rows=0" in L.ncahip_last_error()
    for name in ("source", "target", "proj", "ks", "kt"):
        assert project(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    for name in ("keys", "perm"):
        assert sort(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    for name in ("s", "t", "jmap", "loss", "ws"):
        assert fwd(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    for name in ("s", "t", "jmap", "perm", "proj", "g_loss", "dsource", "ws"):
        assert bwd(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    assert project(ks=a) == -1 and b"alias" in L.ncahip_last_error()
    assert project(kt=d) == -1 and b"alias" in L.ncahip_last_error()
    assert sort(perm=a) == -1 and b"alias" in L.ncahip_last_error()
    assert fwd(loss=a) == -1 and b"alias" in L.ncahip_last_error()
    assert bwd(dsource=a) == -1 and b"alias" in L.ncahip_last_error()
    assert bwd(ws=g) == -1 and b"alias" in L.ncahip_last_error()
    assert project(source=ctypes.c_void_p(0x1004)) == -2 and b"aligned" in L.ncahip_last_error()
    assert fwd(nbytes=L.ncahip_slw_workspace(2, 4, 1000, 1536) - 1) == -1 and b"workspace" in L.ncahip_last_error()
    assert bwd(nbytes=L.ncahip_slw_workspace(2, 64, 1000, 1536) - 1) == -1 and b"workspace" in L.ncahip_last_error()
    assert fwd(B=1, n=1, m=1, nbytes=32 * 4) == -1 and b"workspace" in L.ncahip_last_error()    # the sample sum needs one float more
    with pytest.raises(_capi.NcaHipError):
        _capi.check(-2, "slw_sort")


def test_ops_refuse_cpu_tensors():
    from ncahip import _capi, ops
    z = torch.zeros
    with pytest.raises(_capi.NcaHipError):
        ops.slw_project(z(1, 4, 8), z(1, 4, 8), z(4, 32))
    with pytest.raises(_capi.NcaHipError):
        ops.slw_sort(z(1, 32, 8))
    with pytest.raises(_capi.NcaHipError):
        ops.slw_loss(z(1, 32, 8), z(1, 32, 8), z(8, dtype=torch.int32))
    with pytest.raises(_capi.NcaHipError):
        ops.slw_backward(z(1, 32, 8), z(1, 32, 8), z(8, dtype=torch.int32), z(1, 32, 8, dtype=torch.int32), z(4, 32), z(1))


def _cpu_loss(**kw):
    from ncahip.loss import Loss
    style = (np.random.RandomState(0).rand(48, 48, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Loss(torch.device("cpu"), target_style_image=style, **kw)


def test_slw_impl_accepts_fused_and_refuses_unknown_values():
    assert _cpu_loss(appearance_loss_type="SlW", slw_impl="fused").slw_impl == "fused"
    assert _cpu_loss(appearance_loss_type="SlW").slw_impl == "torch"
    assert _cpu_loss().slw_impl == "torch" and _cpu_loss().ot_impl == "batched"
    with pytest.raises(ValueError):
        _cpu_loss(slw_impl="nope")


def test_fused_loss_refuses_cpu_features_and_other_direction_counts():
    from ncahip import _capi
    from ncahip.loss import sliced_wasserstein_fused
    with pytest.raises(_capi.NcaHipError):
        sliced_wasserstein_fused(torch.zeros(1, 4, 16), torch.zeros(1, 4, 16))
    with pytest.raises(ValueError):
        sliced_wasserstein_fused(torch.zeros(1, 4, 16), torch.zeros(1, 4, 16), n_proj=16)
    L = _cpu_loss(appearance_loss_type="SlW", slw_impl="fused")
    g = torch.Generator().manual_seed(0)
    d = {"generated_images": torch.rand(1, 3, 48, 48, generator=g), "nca_state": torch.rand(1, 16, 48, 48, generator=g),
         "target_images": torch.rand(1, 3, 48, 48, generator=g)}
    with pytest.raises(_capi.NcaHipError):
        L(d)


@pytest.mark.parametrize("m,n", [(50, 37), (1536, 1000), (256, 4096), (4096, 256), (1, 1)])
def test_nearest_index_map_is_interpolates(m, n):
    from ncahip import ops
    jm = ops.slw_nearest_index(m, n)
    assert jm.dtype == torch.int32 and jm.shape == (n,) and int(jm.min()) >= 0 and int(jm.max()) < m
    pt = torch.randn(1, 3, m, generator=torch.Generator().manual_seed(m + n))
    assert torch.equal(pt[:, :, jm.long()], F.interpolate(pt, n, mode="nearest"))
    assert ops.slw_index_map(m, n, "cpu") is ops.slw_index_map(m, n, "cpu")          # built once
    assert torch.equal(ops.slw_index_map(m, n, "cpu"), jm)
