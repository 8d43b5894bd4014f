"""Host-side checks of the fused moment term of the OT loss (no GPU): the new entry points are declared, exported and in the ctypes
table, the workspace size is host arithmetic, argument validation answers before any launch, and the `ot_impl` switch of
ncahip.loss.Loss knows the third value and still refuses an unknown one."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from test_capi_exports import header_prototypes

MOMENT_SYMBOLS = {"ncahip_ot_moment_workspace": 3, "ncahip_ot_moment_fwd_f32": 12, "ncahip_ot_moment_bwd_f32": 10}


def test_symbols_declared_exported_and_bound():
    from ncahip import _capi
    protos = header_prototypes()
    L = _capi.lib()
    for name, nargs in MOMENT_SYMBOLS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert hasattr(L, name), name
        assert len(_capi.SIGNATURES[name]) == nargs, name
    assert _capi.version() == 300


def test_workspace_is_host_arithmetic():
    from ncahip import _capi
    L = _capi.lib()
    # per sample: mx [c], one mean partial per 64-channel tile, one covariance partial per tile pair ti <= tj; floats
    assert L.ncahip_ot_moment_workspace(32, 1000, 512) == 32 * (512 + 8 + 36) * 4
    assert L.ncahip_ot_moment_workspace(1, 2, 4) == (4 + 1 + 1) * 4
    assert L.ncahip_ot_moment_workspace(3, 37, 132) == 3 * (132 + 3 + 6) * 4
    for bad in ((0, 16, 64), (65536, 16, 64), (2, 1, 64), (2, 0, 64), (2, 1025, 64), (2, 16, 516), (2, 16, 6), (2, 16, 0)):
        assert L.ncahip_ot_moment_workspace(*bad) == 0, bad
    assert L.ncahip_ot_workspace(32, 1000, 512) == 2 * 16 * 32 * 1000 * 8        # the relaxed-EMD workspace is what it was


def test_argument_validation_without_gpu():
    from ncahip import _capi
    L = _capi.lib()
    a, b, c, d, e, f, g = (ctypes.c_void_p(0x1000 * n) for n in range(1, 8))      # never dereferenced: every call below is refused
    big = 1 << 30

    def fwd(B=2, N=1000, ch=64, x=a, y=b, mom=c, my=d, sgn=e, S=f, ws=g, nbytes=big):
        return L.ncahip_ot_moment_fwd_f32(x, y, mom, my, sgn, S, B, N, ch, ws, nbytes, None)

    def bwd(B=2, N=1000, ch=64, y=a, my=b, sgn=c, S=d, gm=e, dy=f):
        return L.ncahip_ot_moment_bwd_f32(y, my, sgn, S, gm, dy, B, N, ch, None)

    for call in (fwd, bwd):
        assert call(N=1) == -2 and b"N=1" in L.ncahip_last_error(), call.__name__
        assert call(ch=6) == -2 and b"multiple of 4" in L.ncahip_last_error(), call.__name__
        assert call(ch=516) == -2 and b"512" in L.ncahip_last_error(), call.__name__
        assert call(N=1025) == -2 and b"N=1025" in L.ncahip_last_error(), call.__name__
        assert call(B=65536) == -2 and L.ncahip_last_error(), call.__name__
        assert call(B=0) == -1 and L.ncahip_last_error(), call.__name__
    for name in ("x", "y", "mom", "my", "sgn", "S", "ws"):
        assert fwd(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    for name in ("y", "my", "sgn", "S", "gm", "dy"):
        assert bwd(**{name: None}) == -1 and b"null" in L.ncahip_last_error(), name
    assert fwd(my=a) == -1 and b"alias" in L.ncahip_last_error()                  # an output on an input
    assert fwd(S=b) == -1 and b"alias" in L.ncahip_last_error()
    assert fwd(sgn=d) == -1 and b"alias" in L.ncahip_last_error()                 # two outputs on each other
    assert bwd(dy=a) == -1 and b"alias" in L.ncahip_last_error()
    assert bwd(dy=d) == -1 and b"alias" in L.ncahip_last_error()
    assert fwd(nbytes=L.ncahip_ot_moment_workspace(2, 1000, 64) - 1) == -1 and b"workspace" in L.ncahip_last_error()
    assert fwd(x=ctypes.c_void_p(0x1004)) == -2 and b"aligned" in L.ncahip_last_error()
    assert bwd(dy=ctypes.c_void_p(0x6008)) == -2 and b"aligned" in L.ncahip_last_error()
    with pytest.raises(_capi.NcaHipError):
        _capi.check(-2, "ot_moment_fwd")


def test_ops_refuse_cpu_tensors():
    from ncahip import _capi, ops
    with pytest.raises(_capi.NcaHipError):
        ops.ot_moment(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(_capi.NcaHipError):
        ops.ot_moment_backward(torch.zeros(1, 4, 4), torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4, 4, dtype=torch.int8), torch.zeros(1))


def _cpu_loss(**kw):
    from ncahip.loss import Loss
    style = (np.random.RandomState(0).rand(48, 48, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Loss(torch.device("cpu"), target_style_image=style, **kw)


def test_ot_impl_accepts_fused_all_and_refuses_unknown_values():
    assert _cpu_loss(ot_impl="fused_all").ot_impl == "fused_all"
    assert _cpu_loss().ot_impl == "batched"
    with pytest.raises(ValueError):
        _cpu_loss(ot_impl="bogus")


def test_fused_all_loss_refuses_cpu_features():
    from ncahip import _capi
    from ncahip.loss import ot_loss_fused_all
    with pytest.raises(_capi.NcaHipError):
        ot_loss_fused_all([torch.zeros(1, 4, 4, 4)], [torch.zeros(2, 4, 4, 4)])
    L = _cpu_loss(ot_impl="fused_all")
    g = torch.Generator().manual_seed(0)
    d = {"generated_images": torch.rand(1, 3, 48, 48, generator=g), "nca_state": torch.rand(1, 16, 48, 48, generator=g),
         "target_images": torch.rand(1, 3, 48, 48, generator=g)}
    with pytest.raises(_capi.NcaHipError):
        L(d)
