"""Host-side checks of the fused OT path (no GPU): the new entry points are declared, exported and in the ctypes table, their
argument validation answers before any launch, and the `ot_impl` switch of ncahip.loss.Loss leaves the default path alone."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from test_capi_exports import header_prototypes

OT_SYMBOLS = {"ncahip_ot_workspace": 3, "ncahip_ot_gather_f32": 12, "ncahip_ot_gather_bwd_f32": 8, "ncahip_ot_remd_fwd_f32": 16,
              "ncahip_ot_remd_bwd_f32": 13}


def test_symbols_declared_exported_and_bound():
    from ncahip import _capi
    protos = header_prototypes()
    L = _capi.lib()
    for name, nargs in OT_SYMBOLS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert hasattr(L, name), name
        assert len(_capi.SIGNATURES[name]) == nargs, name
    assert _capi.version() == 300


def test_workspace_is_host_arithmetic():
    from ncahip import _capi
    L = _capi.lib()
    assert L.ncahip_ot_workspace(32, 1000, 512) == 2 * 16 * 32 * 1000 * 8        # one (value, index) per 32-row band and column
    assert L.ncahip_ot_workspace(1, 1, 4) == 2 * 8
    for bad in ((0, 16, 64), (2, 0, 64), (2, 1025, 64), (2, 16, 516), (2, 16, 6)):
        assert L.ncahip_ot_workspace(*bad) == 0, bad


def test_argument_validation_without_gpu():
    from ncahip import _capi
    L = _capi.lib()
    a, b, c, d, e, f, g, h, i, j, k = (ctypes.c_void_p(0x1000 * n) for n in range(1, 12))    # never dereferenced
    big = 1 << 30

    def gather(B=2, ch=64, HW=4096, N=1000, t=a, idx=c):
        return L.ncahip_ot_gather_f32(t, b, idx, d, e, f, g, B, ch, HW, N, None)

    def gather_bwd(B=2, ch=64, HW=4096, N=1000, dy=a):
        return L.ncahip_ot_gather_bwd_f32(dy, b, c, B, ch, HW, N, None)

    def fwd(B=2, N=1000, ch=64, x=a, ws=k, nbytes=big):
        return L.ncahip_ot_remd_fwd_f32(x, b, c, d, e, f, g, h, i, j, B, N, ch, ws, nbytes, None)

    def bwd(B=2, N=1000, ch=64, x=a, dy=i):
        return L.ncahip_ot_remd_bwd_f32(x, b, c, d, e, f, g, h, dy, B, N, ch, None)

    for call in (gather, gather_bwd, fwd, bwd):
        assert call(ch=66) == -2 and b"multiple of 4" in L.ncahip_last_error(), call.__name__
        assert call(ch=516) == -2 and b"512" in L.ncahip_last_error(), call.__name__
        assert call(N=1025) == -2 and b"N=1025" in L.ncahip_last_error(), call.__name__
        assert call(N=0) == -2 and b"N=0" in L.ncahip_last_error(), call.__name__
        assert call(B=0) == -1 and L.ncahip_last_error(), call.__name__
    assert gather(t=None) == -1 and b"null" in L.ncahip_last_error()
    assert gather_bwd(dy=None) == -1 and b"null" in L.ncahip_last_error()
    assert fwd(x=None) == -1 and b"null" in L.ncahip_last_error()
    assert fwd(ws=None) == -1 and b"null" in L.ncahip_last_error()
    assert bwd(x=None) == -1 and b"null" in L.ncahip_last_error()
    assert gather(idx=None) == -1 and b"N == HW" in L.ncahip_last_error()       # no index list means every position
    assert gather(HW=500) == -1                                                 # fewer positions than samples
    assert gather(t=d) == -1 and b"alias" in L.ncahip_last_error()
    assert bwd(dy=a) == -1 and b"alias" in L.ncahip_last_error()
    assert fwd(nbytes=L.ncahip_ot_workspace(2, 1000, 64) - 1) == -1 and b"workspace" in L.ncahip_last_error()
    assert fwd(x=ctypes.c_void_p(0x1004)) == -2 and b"aligned" in L.ncahip_last_error()
    with pytest.raises(_capi.NcaHipError):
        _capi.check(-2, "ot_remd_fwd")


def test_ops_refuse_cpu_tensors():
    from ncahip import _capi, ops
    with pytest.raises(_capi.NcaHipError):
        ops.ot_gather(torch.zeros(1, 4, 2, 2), torch.zeros(2, 4, 2, 2))
    with pytest.raises(_capi.NcaHipError):
        ops.ot_remd(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4), torch.zeros(1, 4))


def _cpu_loss(**kw):
    from ncahip.loss import Loss
    style = (np.random.RandomState(0).rand(48, 48, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return Loss(torch.device("cpu"), target_style_image=style, **kw)


def test_unknown_ot_impl_is_refused():
    with pytest.raises(ValueError):
        _cpu_loss(ot_impl="bogus")


def test_batched_is_the_default_bit_for_bit():
    """ot_impl='batched' is Loss() as it was: same value bits, same position of numpy's global stream afterwards."""
    g = torch.Generator().manual_seed(0)
    d = {"generated_images": torch.rand(2, 3, 80, 80, generator=g), "nca_state": torch.rand(2, 16, 80, 80, generator=g) * 3 - 1.5,
         "target_images": torch.rand(2, 3, 80, 80, generator=g)}
    out = []
    for L in (_cpu_loss(), _cpu_loss(ot_impl="batched")):
        assert L.ot_impl == "batched"
        np.random.seed(5)
        loss, log = L(d)
        st = np.random.get_state()
        out.append((loss.detach().clone(), {k: v.clone() for k, v in log.items()}, st[1].copy(), st[2]))
    (la, ga, ka, pa), (lb, gb, kb, pb) = out
    assert torch.equal(la, lb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert np.array_equal(ka, kb) and pa == pb
    np.random.seed(5)
    assert pa != np.random.get_state()[2] or not np.array_equal(ka, np.random.get_state()[1])   # the 80^2 maps did draw samples


def test_fused_loss_refuses_cpu_features():
    from ncahip import _capi
    L = _cpu_loss(ot_impl="fused")
    g = torch.Generator().manual_seed(0)
    d = {"generated_images": torch.rand(1, 3, 48, 48, generator=g), "nca_state": torch.rand(1, 16, 48, 48, generator=g),
         "target_images": torch.rand(1, 3, 48, 48, generator=g)}
    with pytest.raises(_capi.NcaHipError):
        L(d)
