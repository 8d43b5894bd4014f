"""The standalone kernels of csrc/nca_stencil.hip against float64 at the smallest shape of every class they dispatch to.

Reference, bound and comparator are tests/test_stencil_ref_host.py's (shifted-slice float64 sums on the device, |got - ref| <=
gamma_n A elementwise with A = sum |tap| |input|, nothing excluded, NaN fails); that file proves on the CPU that plain fp32 meets
the bound and that the comparator sees a wrong pad mode, a chunk-local halo row and a wrong wave-edge neighbour.  Nothing here forces
a kernel form: every case reaches its form through the library's own size and alignment rules, so the rules are pinned too.

Every test prints max(err / bound) (-s)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_stencil_ref_host import (DYNCA_FILTERS, EDGE, F64, PADS, ROWS8, SMALL, SOBEL_Y, THRESHOLD, _t, adjoint_abs, check_dynca, compare,
                                   cond_eval, cond_ref, dynca_eval, edge_ref, encoder_ref, gamma, pad_ok, rand, stencil)
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 12345.0

# Which kernel each shape runs, read off the three launchers of csrc/nca_stencil.hip (one thread of a vector form owns 4 W-contiguous
# cells; blocks of 256 threads = 4 waves of 64; a thread takes its left / right cell from lanes -1 / +1 unless it sits in lane 0 / 63,
# is first / last of its row, or is the launch's last thread, and then loads it):
#   nca_launch_dynca_perceive     vec = W % 4 == 0 and x, y 16-byte aligned;  vec and B C H W >= 8 << 20: dynca_perceive_rows_kernel<8>
#                                 (thread = 4 cells x 8 rows, ceil(H / 8) chunks);  vec: dynca_perceive_rows_kernel<1>;  else
#                                 dynca_perceive_scalar_kernel (thread = cell)
#   nca_launch_cond_perceive      vec (same rule, z and y): cond_perceive_kernel<true>;  else cond_perceive_kernel<false>
#   nca_launch_image_encoder_front  ch <= 4: image_encoder_front_kernel<4>;  ch <= 8: <8>;  ch > 8 refused by the C ABI (NCAHIP_ERANGE)
#
#    B   C   H      W      elements       dynca_perceive                                        cond_perceive
# ROWS8 (all four pad modes; reflect not where H < 2)
#    8   16  256    256    8 << 20        rows<8>: bench.py's roofline_stencil call, exactly at the size rule; W/4 = 64, 32 chunks
#    8   32  911    36     8 395 776      rows<8>: W/4 = 9, rows cross wave and block edges at every phase; 114 chunks, last has 7 rows
#    16  64  3      2732   8 392 704      rows<8>: one partial chunk (H < 8, rows 3..7 masked by yy < H); W/4 = 683
#    32  64  1      4096   8 << 20        rows<8>: H = 1, every vertical tap is padding; W/4 = 1024 (whole blocks per row)
#    8   16  16385  4      8 389 120      rows<8>: W/4 = 1, no lane has a neighbour; 2049 chunks, the last holds one row
# THRESHOLD
#    8   16  256    252    8 257 536      rows<1> just under the size rule, W/4 = 63: the wave edge moves one column per wave
#    8   16  256    254    8 323 072      scalar at scale (W % 4 != 0)
# SMALL (dynca_perceive in every pad mode that applies, cond_perceive zero pad)
#    1   1   3      12     36             rows<1>, 9 threads of one wave, 55 inactive lanes clamped to id = 8      <true>, same
#    2   3   5      12     360            rows<1>, W/4 = 3: lane 63 is mid-row in waves 0 and 1                      <true>
#    3   5   7      36     3780           rows<1>, W/4 = 9, 945 threads = 3 full blocks + 177                        <true>
#    1   2   3      260    1560           rows<1>, W/4 = 65: a row longer than a wave                                <true>
#    1   1   2      1028   2056           rows<1>, W/4 = 257: a row longer than a block                              <true>
#    3   5   13     37     9620           scalar, ragged                                                             <false>
#    1   2   9      1      18             scalar, W = 1: every horizontal tap is padding (no reflect)                <false>
# UNALIGNED: (2, 3, 5, 12) and (1, 2, 3, 260) with x (z) or y one float off 16 bytes: scalar / <false> although W % 4 == 0
# ENCODER: (2, ch, 7, 13) and (1, ch, 20, 24); ch = 1, 3, 4: <4>; ch = 5, 8: <8>; ch = 9: NCAHIP_ERANGE, output untouched
# EDGE, ALIVE / FINALIZE: one kernel each (thread = pixel)
ALIVE_SHAPES = [(3, 5, 7, 9), (1, 4, 1, 1), (2, 16, 33, 65)]
UNALIGNED = [(2, 3, 5, 12), (1, 2, 3, 260)]
ADJOINT = [(2, 3, 5, 12), (1, 2, 9, 1)]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops() as o:
        yield o


def _say(case, **kv):
    print(f"\n[ref] {case}: " + ", ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _cases(shapes):
    return [pytest.param(s, p, id=f"{'x'.join(map(str, s))}-{p}") for s in shapes for p in PADS if pad_ok(p, *s[2:])]


def _dynca_case(ops, shape, pad, seed, name):
    x = rand(shape, seed, DEV)
    got = ops.dynca_perceive(x, pad)
    same, bad, worst = check_dynca(got, x, pad)
    _say(f"{name} {shape} {pad}", identity_bit_equal=same, bad=int(bad.sum()), err_over_bound=worst)
    assert got.shape == (shape[0], 4 * shape[1]) + shape[2:]
    assert same and not bool(bad.any()) and worst <= 1.0
    return x, got


# ------------------------------------------------------------------------------------ dynca_perceive
@pytest.mark.parametrize("shape,pad", _cases(ROWS8))
def test_dynca_perceive_rows8(ops, shape, pad):
    B, C, H, W = shape
    assert W % 4 == 0 and B * C * H * W >= 8 << 20            # the size rule of nca_launch_dynca_perceive
    _dynca_case(ops, shape, pad, 1000 + W, "rows<8>")


@pytest.mark.parametrize("pad", PADS)
def test_dynca_perceive_rows8_equals_rows1_bit_for_bit(ops, pad):
    """the benchmark's call (8-row form) against its two B = 4 halves (4 M elements each: the one-row form): the same arithmetic on
    the same nine values"""
    x = rand(ROWS8[0], 1256, DEV)
    full = ops.dynca_perceive(x, pad)
    halves = torch.cat([ops.dynca_perceive(x[:4], pad), ops.dynca_perceive(x[4:], pad)])
    diff = int((full != halves).sum())
    _say(f"rows<8> == rows<1> {ROWS8[0]} {pad}", differing_elements=diff)
    assert torch.equal(full, halves)


@pytest.mark.parametrize("shape,pad", _cases(THRESHOLD))
def test_dynca_perceive_below_the_size_rule(ops, shape, pad):
    B, C, H, W = shape
    assert B * C * H * W < 8 << 20
    _dynca_case(ops, shape, pad, 2000 + W, "rows<1>" if W % 4 == 0 else "scalar")


@pytest.mark.parametrize("shape,pad", _cases(SMALL))
def test_dynca_perceive_small(ops, shape, pad):
    _dynca_case(ops, shape, pad, 3000 + shape[3], "rows<1>" if shape[3] % 4 == 0 else "scalar")


# ------------------------------------------------------------------------------------ cond_perceive
def _cond_check(got, z, wp, name):
    ref, A = cond_ref(z, wp)
    bad, worst = compare(got, ref, gamma(9) * A)
    _say(name, bad=int(bad.sum()), err_over_bound=worst)
    assert not bool(bad.any()) and worst <= 1.0


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_cond_perceive_small(ops, shape):
    z, wp = rand(shape, 4000 + shape[3], DEV), rand((3 * shape[1], 1, 3, 3), 4100 + shape[3], DEV)
    got = ops.cond_perceive(z, wp)
    assert got.shape == (shape[0], 3 * shape[1]) + shape[2:]
    _cond_check(got, z, wp, f"cond_perceive<{'true' if shape[3] % 4 == 0 else 'false'}> {shape}")


# ------------------------------------------------------------------------------------ unaligned pointers
def _carve(n, off):
    """(buffer, view): n floats starting 16 + 4 off bytes into a canary-filled buffer (off = 0: 16-byte aligned, off = 1: not)"""
    buf = torch.full((n + 16,), CANARY, device=DEV)
    view = buf[4 + off:4 + off + n]
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return buf, view


def _canaries_intact(buf, off, n):
    return bool((buf[:4 + off] == CANARY).all()) and bool((buf[4 + off + n:] == CANARY).all())


@pytest.mark.parametrize("which", ["x", "y"])
@pytest.mark.parametrize("shape,pad", _cases(UNALIGNED))
def test_dynca_perceive_unaligned(ops, shape, pad, which):
    """W % 4 == 0 but one pointer off 16 bytes: the scalar form, through the C entry point"""
    from ncahip import _capi
    B, C, H, W = shape
    n = B * C * H * W
    xoff, yoff = (1, 0) if which == "x" else (0, 1)
    xbuf, xv = _carve(n, xoff)
    ybuf, yv = _carve(4 * n, yoff)
    x = rand(shape, 5000 + W, DEV)
    xv.copy_(x.reshape(-1))
    _capi.check(_capi.lib().ncahip_dynca_perceive_f32(xv.data_ptr(), yv.data_ptr(), B, C, H, W, _capi.PAD_MODES[pad], ops._stream()),
                "dynca_perceive")
    torch.cuda.synchronize()
    same, bad, worst = check_dynca(yv.reshape(B, 4 * C, H, W), x, pad)
    _say(f"scalar, {which} unaligned {shape} {pad}", identity_bit_equal=same, bad=int(bad.sum()), err_over_bound=worst)
    assert same and not bool(bad.any()) and worst <= 1.0
    assert _canaries_intact(ybuf, yoff, 4 * n) and _canaries_intact(xbuf, xoff, n)


@pytest.mark.parametrize("which", ["z", "y"])
@pytest.mark.parametrize("shape", UNALIGNED, ids=lambda s: "x".join(map(str, s)))
def test_cond_perceive_unaligned(ops, shape, which):
    from ncahip import _capi
    B, C, H, W = shape
    n = B * C * H * W
    zoff, yoff = (1, 0) if which == "z" else (0, 1)
    zbuf, zv = _carve(n, zoff)
    ybuf, yv = _carve(3 * n, yoff)
    z, wp = rand(shape, 5200 + W, DEV), rand((3 * C, 1, 3, 3), 5300 + W, DEV)
    zv.copy_(z.reshape(-1))
    _capi.check(_capi.lib().ncahip_cond_perceive_f32(zv.data_ptr(), wp.data_ptr(), yv.data_ptr(), B, C, H, W, ops._stream()), "cond_perceive")
    torch.cuda.synchronize()
    _cond_check(yv.reshape(B, 3 * C, H, W), z, wp, f"cond_perceive<false>, {which} unaligned {shape}")
    assert _canaries_intact(ybuf, yoff, 3 * n) and _canaries_intact(zbuf, zoff, n)


# ------------------------------------------------------------------------------------ conditioning front ends
@pytest.mark.parametrize("ch", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("bhw", [(2, 7, 13), (1, 20, 24)], ids=lambda s: "x".join(map(str, s)))
def test_image_encoder_front(ops, bhw, ch):
    B, H, W = bhw
    img, k3, k5 = rand((B, ch, H, W), 6000 + ch, DEV), rand((3, 3, 3), 6100 + ch, DEV), rand((5, 5), 6200 + ch, DEV) * 0.2
    got = ops.image_encoder_front(img, k3, k5)
    ref, bound = encoder_ref(img, k3, k5)
    assert got.shape == ref.shape
    bad_e, worst_e = compare(got[:, :3], ref[:, :3], bound[:, :3])
    bad_b, worst_b = compare(got[:, 3:], ref[:, 3:], bound[:, 3:])
    _say(f"image_encoder_front<{4 if ch <= 4 else 8}> {(B, ch, H, W)}", edges_err_over_bound=worst_e, blur_err_over_bound=worst_b)
    assert not bool(bad_e.any()) and not bool(bad_b.any()) and max(worst_e, worst_b) <= 1.0


def test_image_encoder_front_refuses_nine_channels(ops):
    from ncahip import _capi
    B, ch, H, W = 1, 9, 7, 13
    img, k3, k5 = rand((B, ch, H, W), 6300, DEV), rand((27,), 6301, DEV), rand((25,), 6302, DEV)
    feat = torch.full((B, 3 + ch, H, W), CANARY, device=DEV)
    rc = _capi.lib().ncahip_image_encoder_front_f32(img.data_ptr(), k3.data_ptr(), k5.data_ptr(), feat.data_ptr(), B, ch, H, W, ops._stream())
    torch.cuda.synchronize()
    assert rc == _capi.ERANGE and bool((feat == CANARY).all())


@pytest.mark.parametrize("transform", ["tanh", None])
@pytest.mark.parametrize("shape", EDGE, ids=lambda s: "x".join(map(str, s)))
def test_edge_extractor(ops, shape, transform):
    fixed = torch.tensor([O.SOBEL_X, SOBEL_Y, O.LAPLACIAN], device=DEV)
    for name, k3 in (("fixed", fixed), ("random", rand((3, 3, 3), 6400, DEV))):
        img = rand(shape, 6500 + shape[3], DEV)
        got = ops.edge_extractor(img, k3, transform == "tanh")
        ref, A = edge_ref(img, k3)
        if name == "fixed":
            assert float((ref - O.edge_extractor(img.double(), None)).abs().max()) < 1e-12
        if transform == "tanh":     # tanhf's own error is not derived: the suite's bound
            err = rel_err(got, torch.tanh(ref))
            _say(f"edge_extractor tanh {shape} {name} taps", rel_err=err)
            assert err < 1e-5
        else:
            bad, worst = compare(got, ref, gamma(9) * A)
            _say(f"edge_extractor {shape} {name} taps", bad=int(bad.sum()), err_over_bound=worst)
            assert not bool(bad.any()) and worst <= 1.0


# ------------------------------------------------------------------------------------ alive mask and finalize: exact
def _alpha_planes(shape, thr, seed):
    """three alpha planes [B,1,H,W]: random; below thr with a tenth of the entries exactly float32(thr) (strict >: those cells alone keep
    nobody alive); below thr everywhere except one corner cell, so that only what -inf padding leaves of its 3x3 window is alive"""
    B, _, H, W = shape
    t32 = torch.tensor(thr, dtype=torch.float32, device=DEV)
    rnd = rand((B, 1, H, W), seed, DEV) * 0.5
    below = t32 - 0.01 - rand((B, 1, H, W), seed + 1, DEV).abs()
    at = torch.where(rand((B, 1, H, W), seed + 2, DEV) > 1.2, t32, below)
    at[0, 0, 0, 0] = t32
    corner = below.clone()
    corner[:, 0, H - 1, W - 1] = t32 + 1.0
    return {"random": rnd, "at_thr": at, "corner": corner}


def _alive_torch(x, a, thr):
    if a < 0:
        return torch.ones_like(x[:, :1], dtype=torch.bool)
    return F.max_pool2d(x[:, a:a + 1], 3, 1, 1) > torch.tensor(thr, dtype=torch.float32, device=x.device)   # the ABI takes a float


@pytest.mark.parametrize("shape", ALIVE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cond_alive_and_finalize_exact(ops, shape):
    B, C, H, W = shape
    n = 0
    for a in (-1, 0, C - 1):
        for thr in (0.1, 0.0, -0.5):
            for kind, alpha in _alpha_planes(shape, thr, 7000 + 10 * W).items():
                x = rand(shape, 7100 + W, DEV) * 6.0                      # |x| > 10 at about one entry in ten: both clamps bind
                if a >= 0:
                    x[:, a:a + 1] = alpha
                want_alive = _alive_torch(x, a, thr)
                got_alive = ops.cond_alive(x, a, thr)
                assert got_alive.shape == (B, 1, H, W) and torch.equal(got_alive, want_alive), (a, thr, kind)
                if a >= 0 and kind == "at_thr":
                    assert not bool(want_alive.any())                     # nothing exceeds thr: an `>=` would show
                if a >= 0 and kind == "corner":
                    assert int(want_alive.sum()) == B * min(H, 2) * min(W, 2)
                pre = (rand((B, H, W), 7200 + W, DEV) > -0.5).to(torch.uint8)
                for lo, hi in ((-10.0, 10.0), (-0.25, 0.5)):
                    life = pre.bool()[:, None] & want_alive if a >= 0 else want_alive      # alive_ch < 0: every cell lives, no mask is read
                    want = torch.clamp(x * life, lo, hi)
                    got = ops.cond_finalize(x, pre if a >= 0 else None, a, thr, lo, hi)
                    assert torch.equal(got, want), (a, thr, kind, lo, hi)
                    n += 1
    _say(f"cond_alive / cond_finalize {shape}", exact_cases=n)


# ------------------------------------------------------------------------------------ autograd wrappers
@pytest.mark.parametrize("shape,pad", _cases(ADJOINT))
def test_hip_perceive_gradient(ops, shape, pad):
    """dL/dx of autograd.hip_perceive for a random cotangent: the adjoint of the same linear map, against float64 autograd through the
    shifted-slice reference; bound gamma_9 A^T with A^T = |M|^T |g|"""
    from ncahip import autograd as AG
    x, g = rand(shape, 8000 + shape[3], DEV), rand((shape[0], 4 * shape[1]) + shape[2:], 8100 + shape[3], DEV)
    xr = x.clone().requires_grad_(True)
    y = AG.hip_perceive(xr, pad)
    same, bad, worst_f = check_dynca(y.detach(), x, pad)
    assert same and not bool(bad.any())
    (got,) = torch.autograd.grad(y, xr, g)
    x64 = x.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(dynca_eval(x64, pad), x64, g.double())
    A = adjoint_abs(lambda t: torch.cat([t] + [stencil(t, _t(f, t).abs(), pad) for f in DYNCA_FILTERS], 1), shape, g, DEV)
    bad, worst = compare(got, ref, gamma(9) * A)
    _say(f"hip_perceive {shape} {pad}", forward_err_over_bound=worst_f, grad_bad=int(bad.sum()), grad_err_over_bound=worst)
    assert not bool(bad.any()) and worst <= 1.0


@pytest.mark.parametrize("shape", ADJOINT, ids=lambda s: "x".join(map(str, s)))
def test_hip_cond_perceive_gradient(ops, shape):
    from ncahip import autograd as AG
    C = shape[1]
    z, wp = rand(shape, 8200 + shape[3], DEV), rand((3 * C, 1, 3, 3), 8300 + shape[3], DEV)
    g = rand((shape[0], 3 * C) + shape[2:], 8400 + shape[3], DEV)
    zr, wr = z.clone().requires_grad_(True), wp.clone().requires_grad_(True)
    y = AG._HipCondPerceive.apply(zr, wr)
    _cond_check(y.detach(), z, wp, f"_HipCondPerceive forward {shape}")
    (got,) = torch.autograd.grad(y, zr, g)
    z64 = z.double().requires_grad_(True)
    (ref,) = torch.autograd.grad(cond_eval(z64, wp.double()), z64, g.double())
    A = adjoint_abs(lambda t: cond_eval(t, wp.double().abs()), shape, g, DEV)
    bad, worst = compare(got, ref, gamma(9) * A)
    _say(f"_HipCondPerceive {shape}", grad_bad=int(bad.sum()), grad_err_over_bound=worst)
    assert not bool(bad.any()) and worst <= 1.0
