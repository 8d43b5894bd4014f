"""Host-side checks of the persistent ConditionedNCA grow's C ABI (no GPU): declarations, exports, ctypes arity, the workspace
query and argument refusal before any HIP call."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ncahip.h")
NAMES = ("ncahip_cond_grow_persist_workspace", "ncahip_cond_grow_fwd_persist_f32")


def _lib():
    from ncahip import _capi
    return _capi, _capi.lib()


def _decl_arity(name):
    src = open(HEADER).read()
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def test_header_declares_and_library_exports():
    capi, L = _lib()
    for name in NAMES:
        assert getattr(L, name) is not None
        assert len(capi.SIGNATURES[name]) == _decl_arity(name) == len(getattr(L, name).argtypes), name
    assert capi._RESTYPES["ncahip_cond_grow_persist_workspace"] is ctypes.c_size_t


def test_workspace_query():
    _, L = _lib()
    for shape in ((8, 20, 64, 64, 64, 16), (1, 20, 256, 256, 64, 16), (4, 12, 128, 128, 64, 8)):
        assert L.ncahip_cond_grow_persist_workspace(*shape) > 0, shape
    assert L.ncahip_cond_grow_persist_workspace(8, 20, 40, 64, 64, 16) == 0      # H not a tile multiple
    assert L.ncahip_cond_grow_persist_workspace(8, 24, 64, 64, 64, 16) == 0      # C = 24
    assert L.ncahip_cond_grow_persist_workspace(8, 20, 64, 64, 32, 16) == 0      # hidden != 64


def _call(L, states, ring, T, x_final, C=20, epoch=1, ws=0x100000, nbytes=1 << 24):
    one = ctypes.c_void_p(0x1000)   # never dereferenced: validation fails first
    return L.ncahip_cond_grow_fwd_persist_f32(states, one, ring, T, x_final, None, 0, None, one, one, one, one, one, one,
                                              8, C, 64, 64, 64, 3, 0.1, 0.5, -10.0, 10.0, 0, 0, ctypes.c_void_p(ws), nbytes,
                                              epoch, None)


def test_launch_entry_refuses_before_any_hip_call():
    capi, L = _lib()
    st, xf = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    assert _call(L, st, 3, 5, xf) == capi.EINVAL                         # ring neither 2 nor T + 1
    assert b"ring" in L.ncahip_last_error()
    assert _call(L, st, 2, 5, None) == capi.EINVAL                       # null x_final
    assert b"null" in L.ncahip_last_error()
    assert _call(L, st, 6, 5, xf, C=24) == capi.ERANGE                   # C = 24: not covered
    assert _call(L, st, 2, 5, xf, epoch=0) == capi.EINVAL                # epoch 0
    assert _call(L, st, 2, 4096, xf) == capi.ERANGE                      # T >= 4096
