"""Host-side argument validation of ncahip_cond_fire_words (csrc/nca_capi.hip): every bad argument is refused before any HIP call, so
this runs without a GPU.  The pointers are never dereferenced."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from ncahip import _capi
    return _capi.lib()


WORDS = ctypes.c_void_p(0x1000)


def test_null_words(L):
    from ncahip import _capi
    assert L.ncahip_cond_fire_words(None, 1, 1, 4, 16, 0.5, 0, 0, None) == _capi.EINVAL
    assert b"null" in L.ncahip_last_error()


@pytest.mark.parametrize("Tc,B,H,W", [(0, 1, 4, 16), (-1, 1, 4, 16), (1, 0, 4, 16), (1, 1, 0, 16), (1, 1, 4, 0), (1, -2, 4, 16)])
def test_sizes_must_be_positive(L, Tc, B, H, W):
    from ncahip import _capi
    assert L.ncahip_cond_fire_words(WORDS, Tc, B, H, W, 0.5, 0, 0, None) == _capi.EINVAL
    assert b"positive" in L.ncahip_last_error()


@pytest.mark.parametrize("H,W", [(4, 20), (4, 8), (4, 17), (6, 16), (3, 16), (5, 24)])
def test_whole_tiles_only(L, H, W):
    from ncahip import _capi
    assert L.ncahip_cond_fire_words(WORDS, 1, 1, H, W, 0.5, 0, 0, None) == _capi.ERANGE
    assert b"H % 4 == 0 and W % 16 == 0" in L.ncahip_last_error()


def test_step_count_and_alignment(L):
    from ncahip import _capi
    assert L.ncahip_cond_fire_words(WORDS, 65536, 1, 4, 16, 0.5, 0, 0, None) == _capi.ERANGE
    assert b"65535" in L.ncahip_last_error()
    assert L.ncahip_cond_fire_words(ctypes.c_void_p(0x1004), 1, 1, 4, 16, 0.5, 0, 0, None) == _capi.ERANGE
    assert b"aligned" in L.ncahip_last_error()


def test_the_getter_needs_no_device(L):
    assert L.ncahip_debug_fire_word_launches() >= 0
