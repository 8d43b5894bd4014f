"""Host-side checks of the library's process-wide modes (csrc/nca_modes.h; no GPU): which states keep the persistent ConditionedNCA
grow from running, and that ops.reset_modes() puts everything back.  Only REFUSALS are asserted here: a call that passed the mode
check would go on to launch with the fake pointers below."""
import ctypes
import os
import subprocess
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(TESTS), "video-stylization-with-nca_amd")
B, C, H, W, HIDDEN, T = 1, 16, 16, 16, 64, 4


def refused():
    """One persistent-grow call at 1 x 16 x 16 x 16, hidden 64, T = 4, Philox masks, that is valid but for the modes: True if the library
    refuses it as 'only the default ...' (NCAHIP_ERANGE).  The pointers are never dereferenced."""
    from ncahip import _capi
    L = _capi.lib()
    nbytes = L.ncahip_cond_grow_persist_workspace(B, C, H, W, HIDDEN, 0)
    assert nbytes > 0
    p = lambda a: ctypes.c_void_p(a)      # noqa: E731
    rc = L.ncahip_cond_grow_fwd_persist_f32(p(0x10000), None, 2, T, p(0x20000), None, 0, None, p(0x1000), p(0x1000), p(0x1000), p(0x1000),
                                            p(0x1000), p(0x1000), B, C, H, W, HIDDEN, 3, 0.1, 0.5, -10.0, 10.0, 0, 0, p(0x100000), nbytes, 1,
                                            None)
    # anything else than the refusal would mean the call went past the mode check: stop before another one can
    assert rc == _capi.ERANGE and L.ncahip_last_error().startswith(b"cond grow persist: only the default"), (rc, L.ncahip_last_error())
    return True


@pytest.fixture
def ops():
    from ncahip import ops as _ops
    _ops.reset_modes()
    yield _ops
    _ops.reset_modes()


@pytest.mark.parametrize("bits", [1, 2, 4, 8, 16, 32, 64, 128, 1 << 8, 1 << 16])
def test_every_hook_bit_keeps_the_persistent_grow_from_running(ops, bits):
    ops.force_generic(bits)
    assert refused()


def test_bf16x3_keeps_the_persistent_grow_from_running(ops):
    ops.set_cond_precision(1)
    assert refused()


@pytest.mark.parametrize("var", ["NCAHIP_FORCE_GENERIC", "NCAHIP_COND_VARIANT"])
def test_forward_environment_overrides_keep_it_from_running(var):
    """read when the library is loaded: a fresh process each"""
    code = f"import sys; sys.path[:0] = [{TESTS!r}, {PKG!r}]; import test_modes_host as m; assert m.refused(); print('refused')"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{var: "1"}), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stderr[-2000:]


def test_reset_modes(ops):
    L = ops.lib()
    ops.force_generic(1 | 2 | 4 | 8 | 16 | 32 | 64 | 128 | (3 << 8) | (2 << 16))
    ops.set_cond_precision("bf16x3")
    assert ops.set_dynca_precision("bf16") == "f32"
    assert L.ncahip_debug_persist_drop_tiles(3) == 0
    ops.persistent_steps, ops.persistent_cond = False, True
    ops.reset_modes()
    assert L.ncahip_dynca_precision(0) == 0                      # the previous mode
    assert ops.persistent_steps is True and ops.persistent_cond is False
    assert ops._dynca_direction_cur is None
    ops.force_generic(2)                                         # the hook still works after a reset
    assert refused()
    ops.reset_modes()
