"""Host-side checks of the OT loss's keyed position sampler (no GPU): the numpy mirror ops.ot_sample_idx_host against a literal
restatement of the definition in include/ncahip.h built on the oracle's Philox, the properties of its output, the uniformity of
the definition itself, the C entry point's refusals, and the `idx_source` / `ot_index_rng` plumbing of ncahip.loss on CPU
features."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from test_capi_exports import header_prototypes

OTS = 0x4F5453
SMALL_SHAPES = [(1, 1, 1), (3, 5, 5), (2, 7, 3), (65, 255, 17), (65, 256, 256), (4, 257, 1), (3, 1027, 1), (3, 1027, 1026),
                (2, 1024, 1000), (2, 4096, 1024), (3, 4099, 1000)]
KEY_BITS = (1, 4, 8, 9, 16, 17, 32)


def literal_rows(rows, HW, n, seed, row0, key_bits=32):
    """The definition, row by row: key(p) from the oracle's Philox, np.lexsort((p, key))[:n], sorted."""
    out = np.empty((rows, n), dtype=np.int64)
    p = np.arange(HW, dtype=np.uint64)
    grp = (p >> np.uint64(2)).astype(np.uint32)
    ones = np.ones_like(grp)
    for r in range(rows):
        row = (row0 + r) & (2 ** 64 - 1)
        w = O.philox4x32_10(grp, ones * np.uint32(row & 0xFFFFFFFF), ones * np.uint32(row >> 32), ones * np.uint32(OTS),
                            seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        key = np.stack(w, axis=1)[np.arange(HW), (p & np.uint64(3)).astype(np.int64)].astype(np.uint64) >> np.uint64(32 - key_bits)
        out[r] = np.sort(np.lexsort((p, key))[:n])
    return out


def host(*a, **k):
    from ncahip import ops
    return ops.ot_sample_idx_host(*a, **k)


# ------------------------------------------------------------------ the mirror against the literal restatement
@pytest.mark.parametrize("rows,HW,n", SMALL_SHAPES)
def test_mirror_equals_the_literal_restatement(rows, HW, n):
    for kb in KEY_BITS:
        got = host(rows, HW, n, 0x1234, 7, kb)
        assert got.dtype == np.int32 and got.shape == (rows, n)
        assert np.array_equal(got, literal_rows(rows, HW, n, 0x1234, 7, kb)), (rows, HW, n, kb)


def test_mirror_row_blocks_and_wide_ids():
    # 65 rows of 256 positions; a seed with a high word; ids across the 32-bit boundary
    seed = (0xDEADBEEF << 32) | 0x1234
    assert np.array_equal(host(65, 256, 17, seed, 2 ** 32 - 30, 9), literal_rows(65, 256, 17, seed, 2 ** 32 - 30, 9))


# ------------------------------------------------------------------ output properties
def test_output_properties():
    for rows, HW, n, kb in ((8, 300, 40, 32), (8, 300, 40, 3), (4, 4099, 1000, 32), (4, 64, 63, 1)):
        a = host(rows, HW, n, 5, 0, kb)
        assert a.dtype == np.int32 and a.shape == (rows, n)
        assert (np.diff(a.astype(np.int64), axis=1) > 0).all(), "strictly ascending"
        assert a.min() >= 0 and a.max() < HW
    for kb in (1, 32):
        assert np.array_equal(host(3, 37, 37, 9, 4, kb), np.tile(np.arange(37, dtype=np.int32), (3, 1)))      # n == HW
    a = host(4, 4096, 100, 1, 0)
    assert len({tuple(r) for r in a}) == 4                                                   # rows differ
    assert not np.array_equal(a, host(4, 4096, 100, 2, 0))                                   # seeds differ
    assert np.array_equal(a[1:], host(3, 4096, 100, 1, 1))                                   # row r of a call = row0 + r


def test_row_ids_use_the_high_word():
    base = 2 ** 32 - 2
    four = host(4, 1027, 50, 77, base)
    singles = np.concatenate([host(1, 1027, 50, 77, base + r) for r in range(4)])
    assert np.array_equal(four, singles)
    assert not np.array_equal(four[2:], host(2, 1027, 50, 77, 0)), "ids 2^32 and 2^32 + 1 must not wrap to 0 and 1"


def test_seed_uses_the_high_word():
    lo = 0x89ABCDEF
    assert not np.array_equal(host(2, 1027, 50, (5 << 32) | lo, 0), host(2, 1027, 50, lo, 0))


def test_mirror_refuses_what_the_entry_point_refuses():
    for bad in ((0, 8, 4), (1, 8, 0), (1, 8, 9), (1, 2 ** 20 + 1, 4)):
        with pytest.raises(ValueError):
            host(*bad, 0, 0)
    for kb in (0, 33):
        with pytest.raises(ValueError):
            host(1, 8, 4, 0, 0, kb)


# ------------------------------------------------------------------ uniformity of the definition (deterministic)
@pytest.mark.parametrize("rows,HW,n,seed,kb", [(4096, 64, 16, 1234, 32), (4096, 61, 7, 1234, 32), (4096, 64, 16, 1234, 12)])
def test_inclusion_counts_are_uniform(rows, HW, n, seed, kb):
    """Chi-square of the per-position inclusion counts over rows 0 .. rows - 1, scaled by the finite-population factor of a
    draw without replacement: ~ chi2(HW - 1).  Bound: mean + 5 standard deviations.  Values found: 67.0 / 42.5 / 66.2."""
    count = np.bincount(host(rows, HW, n, seed, 0, kb).ravel(), minlength=HW).astype(np.float64)
    e = rows * n / HW
    stat = float(((count - e) ** 2).sum() / (e * (1.0 - n / HW)))
    bound = (HW - 1) + 5.0 * np.sqrt(2.0 * (HW - 1))
    print(f"rows={rows} HW={HW} n={n} key_bits={kb}: statistic {stat:.1f}, bound {bound:.1f}")
    assert stat < bound, (stat, bound)


def test_adjacent_positions_are_independent():
    """Positions 2k and 2k + 1 take their keys from one Philox call: their co-occurrence count must be what independent
    inclusion gives, rows * 32 * n (n - 1) / (HW (HW - 1)) = 7801.9, within 5 sqrt(expected) ~ 442.  Value found: 7758."""
    rows, HW, n = 4096, 64, 16
    inc = np.zeros((rows, HW), dtype=bool)
    inc[np.arange(rows)[:, None], host(rows, HW, n, 99, 0)] = True
    pairs = int((inc[:, 0::2] & inc[:, 1::2]).sum())
    expected = rows * 32 * n * (n - 1) / (HW * (HW - 1))
    print(f"adjacent pairs: {pairs}, expected {expected:.1f}")
    assert abs(pairs - expected) < 5.0 * np.sqrt(expected), (pairs, expected)


# ------------------------------------------------------------------ the C entry point without a GPU
def test_symbol_declared_exported_and_bound():
    from ncahip import _capi
    assert header_prototypes().get("ncahip_ot_sample_idx") == 8
    assert hasattr(_capi.lib(), "ncahip_ot_sample_idx") and len(_capi.SIGNATURES["ncahip_ot_sample_idx"]) == 8
    assert _capi.version() == 300


def test_argument_validation_without_gpu():
    from ncahip import _capi
    L = _capi.lib()
    buf = ctypes.c_void_p(0x1000)                              # never dereferenced: every call below is refused

    def call(idx=buf, rows=2, HW=4096, n=1000, kb=32):
        return L.ncahip_ot_sample_idx(idx, rows, HW, n, 1, 0, kb, None)

    assert call(idx=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    for kw in ({"rows": 0}, {"rows": -3}, {"HW": 0}, {"n": 0}, {"n": -1}):
        assert call(**kw) == _capi.EINVAL and b"bad size" in L.ncahip_last_error(), kw
    assert call(HW=999) == _capi.EINVAL and b"n=1000 exceeds HW=999" in L.ncahip_last_error()
    assert call(kb=0) == _capi.EINVAL and b"key_bits=0" in L.ncahip_last_error()
    assert call(kb=33) == _capi.EINVAL and b"key_bits=33" in L.ncahip_last_error()
    assert call(n=1025) == _capi.ERANGE and b"n=1025" in L.ncahip_last_error()
    assert call(HW=2 ** 20 + 1) == _capi.ERANGE and b"HW=1048577" in L.ncahip_last_error()
    assert call(rows=65536) == _capi.ERANGE and b"rows=65536" in L.ncahip_last_error()


def test_op_refuses_a_cpu_device():
    from ncahip import _capi, ops
    with pytest.raises(_capi.NcaHipError):
        ops.ot_sample_idx(2, 64, 8, 0, 0, device="cpu")


# ------------------------------------------------------------------ ncahip.loss on CPU features
def _features(B, seed=0):
    """Stand-in style features: a sampled layer (40 x 40, c = 8) and one taken whole (16 x 16, c = 4)."""
    g = torch.Generator().manual_seed(seed)
    target = [torch.rand(1, 8, 40, 40, generator=g), torch.rand(1, 4, 16, 16, generator=g)]
    gen = [torch.rand(B, 8, 40, 40, generator=g), torch.rand(B, 4, 16, 16, generator=g)]
    return target, gen


def _loss(**kw):
    from ncahip.loss import Loss
    return Loss(torch.device("cpu"), content_loss_weight=0.0, appearance_loss_weight=0.0, **kw)      # no VGG: ot_term takes features


def test_idx_source_replaces_the_numpy_draws():
    from ncahip.loss import ot_loss_batched
    target, gen = _features(3)
    seen = []

    def source(li, B, HW, n, device):
        seen.append((li, B, HW, n, torch.device(device).type))
        return torch.from_numpy(host(B, HW, n, 11, li << 16))

    np.random.seed(5)
    before = np.random.get_state()
    v = ot_loss_batched(target, gen, n_samples=100, idx_source=source)
    after = np.random.get_state()
    assert seen == [(0, 3, 1600, 100, "cpu")]                                            # the 16 x 16 layer is not sampled
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "np.random was consumed"
    assert torch.isfinite(v)
    # the same positions, handed over as int64, give the same value
    v64 = ot_loss_batched(target, gen, n_samples=100, idx_source=lambda li, B, HW, n, d: torch.from_numpy(host(B, HW, n, 11, li << 16)).long())
    assert torch.equal(v, v64)
    with pytest.raises(ValueError):
        ot_loss_batched(target, gen, n_samples=100, idx_source=lambda li, B, HW, n, d: torch.zeros(B, n + 1, dtype=torch.int32))


def test_loss_philox_on_cpu_features():
    target, gen = _features(2)
    np.random.seed(7)
    before = np.random.get_state()
    L = _loss(ot_index_rng="philox", ot_index_seed=42)
    assert (L.ot_index_rng, L.ot_index_seed, L.ot_index_call, L.ot_index_offset) == ("philox", 42, 0, 0)
    first, second = L.ot_term(target, gen), L.ot_term(target, gen)
    assert L.ot_index_call == 2
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)), "np.random was consumed"
    assert not torch.equal(first, second), "two consecutive calls must use different positions"

    again = _loss(ot_index_rng="philox", ot_index_seed=42)
    assert torch.equal(again.ot_term(target, gen), first) and torch.equal(again.ot_term(target, gen), second)
    resumed = _loss(ot_index_rng="philox", ot_index_seed=42)
    resumed.ot_index_call = 1
    assert torch.equal(resumed.ot_term(target, gen), second)
    assert not torch.equal(_loss(ot_index_rng="philox", ot_index_seed=43).ot_term(target, gen), first)
    assert not any(k.startswith("ot_index") for k in L.state_dict())

    # the rows are what the docstring says: (call << 24) | (li << 16) | (offset + b)
    from ncahip.loss import ot_loss_batched
    shifted = _loss(ot_index_rng="philox", ot_index_seed=42)
    shifted.ot_index_call, shifted.ot_index_offset = 3, 9
    want = ot_loss_batched(target, gen, idx_source=lambda li, B, HW, n, d: torch.from_numpy(host(B, HW, n, 42, (3 << 24) | (li << 16) | 9)))
    assert torch.equal(shifted.ot_term(target, gen), want)
    shifted.ot_index_offset = 65535
    with pytest.raises(AssertionError):
        shifted.ot_term(target, gen)


def test_unknown_ot_index_rng_is_refused():
    with pytest.raises(ValueError, match="ot_index_rng"):
        _loss(ot_index_rng="bogus")


def test_default_path_is_the_numpy_draw_as_before():
    from ncahip.loss import ot_loss_batched, ot_loss_single
    target, gen = _features(3)
    L = _loss()
    assert L.ot_index_rng == "numpy"
    np.random.seed(21)
    got = L.ot_term(target, gen)
    assert L.ot_index_call == 0
    state = np.random.get_state()
    np.random.seed(21)
    assert torch.equal(got, ot_loss_batched(target, gen))
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state())), "the default path consumes the same draws"
    np.random.seed(21)                                         # ... and they are the reference loop's draws, in its order
    single = sum(ot_loss_single(target, [g[b:b + 1] for g in gen]) for b in range(3)) / 3
    assert abs(float(got) - float(single)) < 1e-4 * abs(float(single))
