"""Host-side checks of the fused-steps path of ncahip_cond_grow_fwd_f32 (csrc/nca_capi.hip): where the per-tile step counters live in
x_final (ncahip_cond_fused_steps_layout: the arithmetic the grow itself uses), argument validation, and the hook bits.  Nothing is
launched, so this runs without a GPU; the pointers handed to the library are host memory it only writes three numbers to."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from ncahip import _capi
    return _capi.lib()


def _layout(L, B, C, H, W, cap=0):
    chunk, off, nbytes = ctypes.c_int(-1), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = L.ncahip_cond_fused_steps_layout(B, C, H, W, cap, ctypes.byref(chunk), ctypes.byref(off), ctypes.byref(nbytes))
    return rc, chunk.value, off.value, nbytes.value


@pytest.mark.parametrize("B,C,H,W", [(8, 16, 256, 256), (2, 16, 48, 64), (3, 12, 12, 48), (2, 10, 16, 32), (1, 1, 4, 16), (3, 14, 48, 64),
                                     (1, 16, 2048, 2048)])
def test_words_and_counters_fit_x_final(L, B, C, H, W):
    rc, chunk, off, nbytes = _layout(L, B, C, H, W)
    assert rc == 0
    slot, words = B * C * H * W * 4, B * H * W // 8           # bytes of x_final / of one step's fire words
    tiles = B * (H // 4) * (W // 16)
    assert nbytes >= 4 * (tiles + 1) and nbytes % 64 == 0 and nbytes < 4 * (tiles + 1) + 64   # the counters and the abort word
    assert off == chunk * words and off % 8 == 0              # behind the words, aligned for 32-bit counters
    assert off + nbytes <= slot                               # inside x_final
    assert 1 <= chunk <= 32 * C
    assert (chunk + 1) * words + nbytes > slot                # and no step fewer than fits
    assert chunk == 32 * C - -(-nbytes // words)              # the words alone fill x_final at 32 C steps: the counters cost one (tiny grids: a few)


@pytest.mark.parametrize("cap", [1, 4, 255])
def test_chunk_cap(L, cap):
    rc, chunk, off, nbytes = _layout(L, 2, 16, 48, 64, cap)
    assert rc == 0 and chunk == min(cap, 32 * 16 - 1) and off == chunk * (2 * 48 * 64 // 8)


def test_null_pointers(L):
    from ncahip import _capi
    c, o, n = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
    assert L.ncahip_cond_fused_steps_layout(1, 16, 4, 16, 0, None, ctypes.byref(o), ctypes.byref(n)) == _capi.EINVAL
    assert L.ncahip_cond_fused_steps_layout(1, 16, 4, 16, 0, ctypes.byref(c), None, ctypes.byref(n)) == _capi.EINVAL
    assert L.ncahip_cond_fused_steps_layout(1, 16, 4, 16, 0, ctypes.byref(c), ctypes.byref(o), None) == _capi.EINVAL
    assert b"null" in L.ncahip_last_error()


@pytest.mark.parametrize("B,C,H,W,cap", [(0, 16, 4, 16, 0), (1, 0, 4, 16, 0), (1, 16, 0, 16, 0), (1, 16, 4, 0, 0), (-1, 16, 4, 16, 0),
                                         (1, 16, 4, 16, -1)])
def test_sizes_must_be_positive(L, B, C, H, W, cap):
    from ncahip import _capi
    rc, chunk, _, _ = _layout(L, B, C, H, W, cap)
    assert rc == _capi.EINVAL and chunk == -1
    assert b"positive" in L.ncahip_last_error()


@pytest.mark.parametrize("H,W", [(4, 20), (4, 8), (6, 16), (3, 16), (5, 24)])
def test_whole_tiles_only(L, H, W):
    from ncahip import _capi
    rc, chunk, _, _ = _layout(L, 1, 16, H, W)
    assert rc == _capi.ERANGE and chunk == -1
    assert b"H % 4 == 0 and W % 16 == 0" in L.ncahip_last_error()


def test_hook_bits_and_getter_need_no_device(L):
    from ncahip import ops
    assert ops.NO_FUSED_STEPS == 1 << 24 and ops.FUSED_STEPS_CAP_SHIFT == 25
    ops.force_generic(ops.NO_FUSED_STEPS | (3 << ops.FUSED_STEPS_CAP_SHIFT))
    ops.reset_modes()                                          # force_generic(0): the off switch and the cap are hook bits
    assert L.ncahip_debug_fused_step_launches() >= 0
    assert ops.fused_step_launches() >= 0
