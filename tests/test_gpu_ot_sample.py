"""The OT loss's keyed position sampler on the device (csrc/nca_ot_sample.hip, ops.ot_sample_idx) against its numpy mirror
ops.ot_sample_idx_host -- which tests/test_ot_sample_host.py holds against a literal restatement of the definition built on the
oracle's Philox -- and the `idx_source` / `ot_index_rng` plumbing of ncahip.loss on CUDA features: equal positions must give equal
bits, because the OT kernels are bit-reproducible."""
import numpy as np
import pytest
import torch

from gpu_ops import gpu_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (3, 1027, 1026) asks for more than the entry point's 1024 positions per row (the gather's limit): there the refusal is what is
# checked -- the mirror takes that shape in tests/test_ot_sample_host.py -- and (3, 1027, 1024) / (3, 1025, 1024) stand next to it as
# the largest n at that HW and n = HW - 1 at the limit.
SHAPES = [(1, 1, 1), (3, 5, 5), (2, 7, 3), (65, 255, 17), (65, 256, 256), (4, 257, 1), (3, 1027, 1), (3, 1027, 1026), (3, 1027, 1024),
          (3, 1025, 1024), (2, 1024, 1000), (2, 4096, 1024), (3, 4099, 1000)]
KEY_BITS = (1, 4, 8, 9, 16, 17, 32)


@pytest.fixture(scope="module")
def ops():
    with gpu_ops() as o:
        o.check_errors()
        yield o


def mirror(ops, *a, **k):
    return torch.from_numpy(ops.ot_sample_idx_host(*a, **k))


# ------------------------------------------------------------------ the kernel against the mirror
@pytest.mark.parametrize("rows,HW,n", SHAPES)
def test_kernel_equals_the_mirror(ops, rows, HW, n):
    if n > 1024:
        from ncahip._capi import NcaHipError
        for kb in KEY_BITS:
            with pytest.raises(NcaHipError, match=f"rc=-2.*n={n}"):
                ops.ot_sample_idx(rows, HW, n, 0x1234, 7, kb, device=DEV)
        return
    got = [ops.ot_sample_idx(rows, HW, n, 0x1234, 7, kb, device=DEV) for kb in KEY_BITS]       # enqueue all, then compare
    for kb, g in zip(KEY_BITS, got):
        assert g.dtype == torch.int32 and g.shape == (rows, n) and g.device == torch.device(DEV)
        assert torch.equal(g.cpu(), mirror(ops, rows, HW, n, 0x1234, 7, kb)), (rows, HW, n, kb)
    ops.check_errors()


def test_row_ids_and_seed_use_their_high_words(ops):
    base = 2 ** 32 - 2
    got = ops.ot_sample_idx(4, 1027, 50, 77, base, device=DEV).cpu()
    assert torch.equal(got, mirror(ops, 4, 1027, 50, 77, base))
    assert torch.equal(got[2:], ops.ot_sample_idx(2, 1027, 50, 77, 2 ** 32, device=DEV).cpu())
    seed = (0xDEADBEEF << 32) | 0x89ABCDEF
    hi = ops.ot_sample_idx(3, 1027, 50, seed, 5, device=DEV).cpu()
    assert torch.equal(hi, mirror(ops, 3, 1027, 50, seed, 5))
    assert not torch.equal(hi, ops.ot_sample_idx(3, 1027, 50, seed & 0xFFFFFFFF, 5, device=DEV).cpu())


def test_non_default_stream(ops):
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        got = ops.ot_sample_idx(5, 4099, 1000, 3, 11, device=DEV)
    s.synchronize()
    assert torch.equal(got.cpu(), mirror(ops, 5, 4099, 1000, 3, 11))


@pytest.mark.parametrize("HW", [65536, 262144])
def test_full_size_row(ops, HW):
    got = ops.ot_sample_idx(1, HW, 1000, 2024, (3 << 24) | (1 << 16), device=DEV).cpu()
    assert torch.equal(got, mirror(ops, 1, HW, 1000, 2024, (3 << 24) | (1 << 16)))
    ops.check_errors()


def test_canary_on_both_sides(ops):
    from ncahip._capi import check
    rows, HW, n, pad = 3, 4099, 1000, 256
    for kb in (32, 2):
        big = torch.full((pad + rows * n + pad,), -7, dtype=torch.int32, device=DEV)
        check(ops.lib().ncahip_ot_sample_idx(big[pad:].data_ptr(), rows, HW, n, 9, 0, kb, ops._stream()), "ot_sample_idx")
        big = big.cpu()
        assert bool((big[:pad] == -7).all()) and bool((big[pad + rows * n:] == -7).all())
        assert torch.equal(big[pad:pad + rows * n].reshape(rows, n), mirror(ops, rows, HW, n, 9, 0, kb))


def test_sticky_error_word_refuses_the_sampler(ops):
    from ncahip._capi import NcaHipError
    ops.check_errors()
    assert ops.lib().ncahip_debug_inject_error(1) == 0
    try:
        with pytest.raises(NcaHipError, match="device-side failure"):
            ops.ot_sample_idx(2, 4096, 1000, 0, 0, device=DEV)
    finally:
        ops.lib().ncahip_check_errors(ops._stream(), 1)      # never leave the word set for later tests
    ops.check_errors()
    assert torch.equal(ops.ot_sample_idx(2, 4096, 1000, 0, 0, device=DEV).cpu(), mirror(ops, 2, 4096, 1000, 0, 0))


# ------------------------------------------------------------------ end to end through ncahip.loss
def _features(B, c, seed=0):
    """Stand-in style features: a sampled layer (40 x 40, n = 1000) and one taken whole (16 x 16).  Strictly positive: an all-zero
    feature vector (one in 50 of relu(randn + 0.3) at c = 4) makes the torch path's gradient NaN (ncahip.loss.ot_loss_fused's
    docstring), and NaN never compares equal."""
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: (torch.rand(*s, generator=g) + 0.05).to(DEV)
    return [f(1, c, 40, 40), f(1, c, 16, 16)], [f(B, c, 40, 40), f(B, c, 16, 16)]


def _value_and_grads(fn, target, gen, **kw):
    leaves = [g.clone().requires_grad_(True) for g in gen]
    v = fn(target, leaves, **kw)
    v.backward()
    return v.detach(), [x.grad for x in leaves]


@pytest.mark.parametrize("c", [4, 64])
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("impl", ["batched", "fused", "fused_all"])
def test_loss_with_device_indices_equals_uploaded_mirror_indices(ops, impl, B, c):
    from ncahip.loss import _OT_IMPLS
    target, gen = _features(B, c, seed=B * 100 + c)
    seed, call = 31, 6
    row0 = lambda li: (call << 24) | (li << 16)
    on_device = lambda li, B_, HW, n, dev: ops.ot_sample_idx(B_, HW, n, seed, row0(li), device=dev)
    uploaded = lambda li, B_, HW, n, dev: mirror(ops, B_, HW, n, seed, row0(li)).to(dev)
    np.random.seed(3)
    before = np.random.get_state()
    v0, g0 = _value_and_grads(_OT_IMPLS[impl], target, gen, idx_source=on_device)
    v1, g1 = _value_and_grads(_OT_IMPLS[impl], target, gen, idx_source=uploaded)
    assert all(np.array_equal(a, b) for a, b in zip(before, np.random.get_state())), "np.random was consumed"
    assert bool(torch.isfinite(v0)) and torch.equal(v0, v1)
    for a, b in zip(g0, g1):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert int((g0[0].reshape(B, c, -1).abs().sum(1) != 0).sum(1).max()) <= 1000        # only sampled positions carry a gradient
    ops.check_errors()


@pytest.mark.parametrize("impl", ["batched", "fused", "fused_all"])
def test_loss_object_with_philox_indices(ops, impl):
    from ncahip.loss import _OT_IMPLS, Loss
    B, c = 2, 64
    target, gen = _features(B, c, seed=8)
    L = Loss(torch.device(DEV), content_loss_weight=0.0, appearance_loss_weight=0.0, ot_impl=impl, ot_index_rng="philox", ot_index_seed=17)
    L.ot_index_call, L.ot_index_offset = 4, 3
    np.random.seed(3)
    before = np.random.get_state()
    leaves = [g.clone().requires_grad_(True) for g in gen]
    v = L.ot_term(target, leaves)
    v.backward()
    assert L.ot_index_call == 5
    assert all(np.array_equal(a, b) for a, b in zip(before, np.random.get_state())), "np.random was consumed"
    uploaded = lambda li, B_, HW, n, dev: mirror(ops, B_, HW, n, 17, (4 << 24) | (li << 16) | 3).to(dev)
    v1, g1 = _value_and_grads(_OT_IMPLS[impl], target, gen, idx_source=uploaded)
    assert torch.equal(v.detach(), v1) and all(bool(torch.isfinite(b).all()) and torch.equal(x.grad, b) for x, b in zip(leaves, g1))
    ops.check_errors()


def test_philox_value_is_finite_and_repeatable(ops):
    """fused_all with numpy positions and with philox positions are two samples of one estimator: no closeness is asserted (it
    would be a statistical guess), only that the philox value is finite and that equal (seed, call) give equal bits."""
    from ncahip.loss import Loss
    target, gen = _features(3, 64, seed=9)
    L = Loss(torch.device(DEV), content_loss_weight=0.0, appearance_loss_weight=0.0, ot_impl="fused_all", ot_index_rng="philox", ot_index_seed=5)
    a = L.ot_term(target, gen)
    b = L.ot_term(target, gen)
    L.ot_index_call = 0
    a2 = L.ot_term(target, gen)
    assert bool(torch.isfinite(a)) and bool(torch.isfinite(b))
    assert torch.equal(a, a2) and not torch.equal(a, b)
    np.random.seed(0)
    default = Loss(torch.device(DEV), content_loss_weight=0.0, appearance_loss_weight=0.0, ot_impl="fused_all").ot_term(target, gen)
    print(f"fused_all OT term: philox {float(a):.6f} / {float(b):.6f}, numpy {float(default):.6f}")
    assert bool(torch.isfinite(default))
    ops.check_errors()
