"""The float64 reference, the error bound and the comparator that tests/test_gpu_stencil_ref.py holds the standalone kernels of
csrc/nca_stencil.hip to, checked on the CPU: the reference against the oracle, the bound against plain fp32 evaluations of the same
sums, and the comparator against the mistakes it exists to catch.

Reference.  stencil() pads with F.pad(x, [r, r, r, r], mode) and sums the k x k shifted slices times the taps, in the dtype and on
the device of its input; no F.conv2d.  Fed |x| and |w| the same routine gives A = sum_t |w_t| |x_t| per output element.

Bound.  For an n-term fp32 dot product evaluated in any order, with or without FMA, |got - ref| <= gamma_n A with gamma_n =
n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The float64 reference's own
error, about 2^-53 A, is 2^-29 of that.  Applied elementwise, nothing excluded, NaN fails:
    dynca_perceive      identity plane bit-equal to x; Sobel x, Sobel y, Laplacian within gamma_9 A (the fixed taps 1, 2, 12 are
                        exact, a product by 2 does not round, so the kernel's factored forms stay inside the 9-term bound)
    cond_perceive       gamma_9 A, arbitrary fp32 taps
    image_encoder_front blur planes gamma_25 A; edge planes gamma_{ch+11} sum_t |k3_t| mean_c |img_t|: ch - 1 additions for the
                        channel sum, two roundings for the product with the rounded 1 / ch (or one for a true division), nine terms
    edge_extractor      gamma_9 A without tanh; with tanh the suite's rel_err < 1e-5 (tanhf's own error is not derived here)
    adjoints            the gradient of a linear map for a cotangent g is the same kind of sum with x and g exchanged: gamma_9 A^T,
                        A^T = |M|^T |g| (adjoint_abs)
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O

F64 = torch.float64
U = 2.0 ** -24
PADS = O.PAD_MODES                          # "constant", "replicate", "circular", "reflect": F.pad's own names
SOBEL_Y = [list(r) for r in zip(*O.SOBEL_X)]
DYNCA_FILTERS = (O.SOBEL_X, SOBEL_Y, O.LAPLACIAN)

# every small shape of the GPU file (B, C, H, W) and every large one; the CPU evaluates the large ones on a band of rows
SMALL = [(1, 1, 3, 12), (2, 3, 5, 12), (3, 5, 7, 36), (1, 2, 3, 260), (1, 1, 2, 1028), (3, 5, 13, 37), (1, 2, 9, 1)]
ROWS8 = [(8, 16, 256, 256), (8, 32, 911, 36), (16, 64, 3, 2732), (32, 64, 1, 4096), (8, 16, 16385, 4)]
THRESHOLD = [(8, 16, 256, 252), (8, 16, 256, 254)]
ENCODER = [(2, ch, 7, 13) for ch in (1, 3, 4, 5, 8)] + [(1, ch, 20, 24) for ch in (1, 3, 4, 5, 8)]
EDGE = [(2, 1, 9, 31), (1, 1, 1, 1)]
BAND_ROWS = 24


def gamma(n):
    return n * U / (1.0 - n * U)


def pad_ok(pad, H, W):
    return pad != "reflect" or (H >= 2 and W >= 2)     # F.pad and the C ABI both refuse reflect on a one-cell axis


def rand(shape, seed, device="cpu"):
    return torch.randn(*shape, generator=torch.Generator(device=device).manual_seed(seed), device=device)


# ------------------------------------------------------------------------------------ reference
def stencil(x, w, mode="constant"):
    """sum_{dy,dx} w[..., dy, dx] * pad(x)[.., y + dy, x + dx]: x [B,C,H,W], w [k,k] or [C,k,k] (k odd), F.pad mode"""
    k = w.shape[-1]
    r = k // 2
    H, W = x.shape[-2:]
    xp = F.pad(x, [r, r, r, r], mode)
    w = w.to(x.dtype).to(x.device)
    out = torch.zeros(x.shape, dtype=x.dtype, device=x.device)
    for dy in range(k):
        for dx in range(k):
            t = w[..., dy, dx]
            out += (t.reshape(1, -1, 1, 1) if t.dim() else t) * xp[:, :, dy:dy + H, dx:dx + W]
    return out


def stencil_ref(x, w, mode="constant"):
    """(float64 reference, A) of one filter (bank)"""
    x, w = x.to(F64), w.to(F64)
    return stencil(x, w, mode), stencil(x.abs(), w.abs(), mode)


def _t(f, like):
    return torch.tensor(f, dtype=like.dtype, device=like.device)


def dynca_planes(x, pad):
    """yields (f, reference, A) for the Sobel x, Sobel y and Laplacian plane groups f = 1, 2, 3 of [x | Sx x | Sy x | L x], one at a
    time (the large shapes hold one group of float64 at once)"""
    for f, filt in enumerate(DYNCA_FILTERS, 1):
        yield (f,) + stencil_ref(x, _t(filt, x), pad)


def dynca_eval(x, pad):
    """[x | Sx x | Sy x | L x] by shifted slices in x's dtype"""
    return torch.cat([x] + [stencil(x, _t(f, x), pad) for f in DYNCA_FILTERS], 1)


def cond_w(wp, C):
    return wp.reshape(3 * C, 3, 3)


def cond_eval(z, wp):
    """perception_net: output channel 3 c + k is filter wp[3 c + k] on input channel c, zero pad"""
    C = z.shape[1]
    return stencil(z.repeat_interleave(3, 1), cond_w(wp, C).to(z.dtype))


def cond_ref(z, wp):
    return stencil_ref(z.repeat_interleave(3, 1), cond_w(wp, z.shape[1]))


def edge_ref(img, k3):
    """[B,1,H,W], k3 [3,3,3] -> (ref, A) [B,3,H,W], zero pad, before the transform"""
    return stencil_ref(img.expand(-1, 3, -1, -1), k3.reshape(3, 3, 3))


def encoder_ref(img, k3, k5):
    """image_encoder_front [sx | sy | lap | blur(ch)]: (ref, bound) with the bounds of the table above"""
    ch = img.shape[1]
    i64 = img.to(F64)
    e, _ = stencil_ref(i64.mean(1, keepdim=True).expand(-1, 3, -1, -1), k3.reshape(3, 3, 3))
    ea = stencil(i64.abs().mean(1, keepdim=True).expand(-1, 3, -1, -1), k3.reshape(3, 3, 3).to(F64).abs())
    b, ba = stencil_ref(i64, k5.reshape(5, 5))
    return torch.cat([e, b], 1), torch.cat([gamma(ch + 11) * ea, gamma(25) * ba], 1)


def adjoint_abs(fwd_abs, x_shape, g, device):
    """|M|^T |g| for the linear map x -> fwd_abs(x) (the map with |taps|), by float64 autograd"""
    x = torch.zeros(*x_shape, dtype=F64, device=device, requires_grad=True)
    (a,) = torch.autograd.grad(fwd_abs(x), x, g.to(F64).abs())
    return a


# ------------------------------------------------------------------------------------ comparator
def compare(got, ref, bound):
    """(bad, worst): bad marks every element with not |got - ref| <= bound (NaN fails), worst = max err / bound (inf where the
    bound is zero and the error is not)"""
    err = (got.to(F64) - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    return bad, float(ratio.max()) if ratio.numel() else 0.0


def check_dynca(got, x, pad):
    """got [B,4C,H,W] against the float64 reference of x: (identity plane bit-equal, bad [B,3C,H,W], worst err / bound)"""
    C = x.shape[1]
    bads, worst = [], 0.0
    for f, ref, A in dynca_planes(x, pad):
        bad, w = compare(got[:, f * C:(f + 1) * C], ref, gamma(9) * A)
        bads.append(bad)
        worst = max(worst, w)
    return torch.equal(got[:, :C], x), torch.cat(bads, 1), worst


def border(shape, device="cpu"):
    """[H,W] bool: cells within one cell of the border"""
    H, W = shape[-2:]
    m = torch.ones(H, W, dtype=torch.bool, device=device)
    m[1:-1, 1:-1] = False
    return m


def band(shape):
    B, C, H, W = shape
    return (1, 2, min(H, BAND_ROWS), W)


def _shapes_cpu():
    return SMALL + [band(s) for s in ROWS8 + THRESHOLD]


# ------------------------------------------------------------------------------------ 1. the reference is the oracle's map
@pytest.mark.parametrize("pad", PADS)
def test_reference_equals_oracle_dynca(pad):
    for i, shape in enumerate(SMALL):
        if not pad_ok(pad, *shape[2:]):
            continue
        x = rand(shape, 10 + i).to(F64)
        ref = dynca_eval(x, pad)
        assert float((ref - O.dynca_perceive(x, pad)).abs().max()) < 1e-12, shape
    x = rand((2, 3, 5, 6), 3).to(F64)
    assert float((dynca_eval(x, pad) - torch.from_numpy(O.dynca_perceive_np(x.numpy(), pad))).abs().max()) < 1e-12


def test_reference_equals_oracle_cond_and_edges():
    for i, shape in enumerate(SMALL):
        z, wp = rand(shape, 20 + i).to(F64), rand((3 * shape[1], 1, 3, 3), 40 + i).to(F64)
        assert float((cond_eval(z, wp) - O.cond_perceive(z, wp)).abs().max()) < 1e-12, shape
    k3 = torch.tensor([O.SOBEL_X, SOBEL_Y, O.LAPLACIAN])
    for i, shape in enumerate(EDGE):
        img = rand(shape, 60 + i).to(F64)
        assert float((edge_ref(img, k3)[0] - O.edge_extractor(img, None)).abs().max()) < 1e-12, shape


def test_reference_equals_oracle_encoder_front():
    """the fixed-filter front of O.image_encoder: gray -> three 3x3 filters, per-channel 5x5 blur"""
    k3 = torch.tensor([O.SOBEL_X, SOBEL_Y, O.LAPLACIAN]).to(F64)
    k5 = O.gaussian_kernel_5x5(1.0).to(F64)
    for i, shape in enumerate(ENCODER):
        img = rand(shape, 80 + i).to(F64)
        gray = img.mean(1, keepdim=True)
        want = torch.cat([F.conv2d(gray, k3[:, None], padding=1)] + [F.conv2d(img[:, c:c + 1], k5, padding=2) for c in range(shape[1])], 1)
        assert float((encoder_ref(img, k3, k5)[0] - want).abs().max()) < 1e-12, shape


# ------------------------------------------------------------------------------------ 2. plain fp32 meets the bound everywhere
@pytest.mark.parametrize("pad", PADS)
def test_fp32_evaluations_meet_the_dynca_bound(pad):
    for i, shape in enumerate(_shapes_cpu()):
        if not pad_ok(pad, *shape[2:]):
            continue
        x = rand(shape, 100 + i)
        for name, got in (("conv", O.dynca_perceive(x, pad)), ("slices", dynca_eval(x, pad))):
            same, bad, worst = check_dynca(got, x, pad)
            assert same and not bool(bad.any()) and worst <= 1.0, (name, shape, worst)


def test_fp32_evaluations_meet_the_cond_and_edge_bounds():
    for i, shape in enumerate(SMALL):
        z, wp = rand(shape, 120 + i), rand((3 * shape[1], 1, 3, 3), 140 + i)
        ref, A = cond_ref(z, wp)
        for name, got in (("conv", O.cond_perceive(z, wp)), ("slices", cond_eval(z, wp))):
            bad, worst = compare(got, ref, gamma(9) * A)
            assert not bool(bad.any()) and worst <= 1.0, (name, shape, worst)
    for i, shape in enumerate(EDGE):
        img, k3 = rand(shape, 160 + i), rand((3, 3, 3), 170 + i)
        ref, A = edge_ref(img, k3)
        for name, got in (("conv", F.conv2d(img, k3[:, None], padding=1)), ("slices", stencil(img.expand(-1, 3, -1, -1), k3))):
            bad, worst = compare(got, ref, gamma(9) * A)
            assert not bool(bad.any()) and worst <= 1.0, (name, shape, worst)


def test_fp32_evaluations_meet_the_encoder_bounds():
    for i, shape in enumerate(ENCODER):
        ch = shape[1]
        img, k3, k5 = rand(shape, 180 + i), rand((3, 3, 3), 200 + i), rand((5, 5), 220 + i) * 0.2
        ref, bound = encoder_ref(img, k3, k5)
        gray = img.mean(1, keepdim=True)                                       # sum / ch
        grayi = img.sum(1, keepdim=True) * torch.tensor(1.0 / ch, dtype=torch.float32)   # sum * fl(1 / ch), the kernel's form
        for name, g in (("div", gray), ("inv", grayi)):
            got = torch.cat([F.conv2d(g, k3[:, None], padding=1), stencil(img, k5)], 1)
            bad, worst = compare(got, ref, bound)
            assert not bool(bad.any()) and worst <= 1.0, (name, shape, worst)


def test_fp32_adjoints_meet_the_bound():
    """gradient of the fp32 maps for a random cotangent against float64 autograd through the shifted-slice reference"""
    for shape in ((2, 3, 5, 12), (1, 2, 9, 1)):
        for pad in PADS:
            if not pad_ok(pad, *shape[2:]):
                continue
            x, g = rand(shape, 240), rand((shape[0], 4 * shape[1]) + shape[2:], 241)
            got = _grad(lambda t: dynca_eval(t, pad), x, g)
            ref = _grad(lambda t: dynca_eval(t, pad), x.to(F64), g.to(F64))
            A = adjoint_abs(lambda t: torch.cat([t] + [stencil(t, _t(f, t).abs(), pad) for f in DYNCA_FILTERS], 1), shape, g, "cpu")
            bad, worst = compare(got, ref, gamma(9) * A)
            assert not bool(bad.any()), (shape, pad, worst)
        z, wp, g = rand(shape, 250), rand((3 * shape[1], 1, 3, 3), 251), rand((shape[0], 3 * shape[1]) + shape[2:], 252)
        got = _grad(lambda t: cond_eval(t, wp), z, g)
        ref = _grad(lambda t: cond_eval(t, wp.to(F64)), z.to(F64), g.to(F64))
        A = adjoint_abs(lambda t: cond_eval(t, wp.to(F64).abs()), shape, g, "cpu")
        bad, worst = compare(got, ref, gamma(9) * A)
        assert not bool(bad.any()), (shape, worst)


def _grad(fn, x, g):
    x = x.detach().clone().requires_grad_(True)
    return torch.autograd.grad(fn(x), x, g)[0]


# ------------------------------------------------------------------------------------ 3. the comparator catches what it is for
def test_comparator_catches_one_moved_element():
    x = rand((2, 3, 5, 12), 300)
    idx = (1, 2, 2, 11)
    for pad in PADS:
        got = dynca_eval(x, pad).to(F64)
        for f, ref, A in dynca_planes(x, pad):
            g = got[:, f * 3:(f + 1) * 3].clone()
            assert not bool(compare(g, ref, gamma(9) * A)[0].any())
            assert float(A[idx]) > 0
            g[idx] += 4 * gamma(9) * A[idx]
            bad, worst = compare(g, ref, gamma(9) * A)
            assert int(bad.sum()) == 1 and bool(bad[idx]) and 3.0 <= worst <= 5.0, (pad, f)
            g[idx] = float("nan")
            bad, worst = compare(g, ref, gamma(9) * A)
            assert int(bad.sum()) == 1 and bool(bad[idx]) and worst == float("inf"), (pad, f)      # NaN fails
    y = dynca_eval(x, "replicate")
    y[1, 1, 3, 7] = torch.nextafter(y[1, 1, 3, 7], torch.tensor(float("inf")))
    assert not check_dynca(y, x, "replicate")[0]                   # the identity plane is held to the bit


@pytest.mark.parametrize("pad", PADS)
def test_comparator_catches_every_other_pad_mode(pad):
    shape = (2, 3, 5, 12)
    x = rand(shape, 310)
    got = dynca_eval(x, pad)
    ring = border(shape)
    for other in PADS:
        same, bad, worst = check_dynca(got, x, other)
        if other == pad:
            assert same and not bool(bad.any())
            continue
        assert bool(bad.any()) and worst > 1.0, (pad, other)
        assert not bool((bad & ~ring).any()), (pad, other)            # and only where the padding is read
        for f in range(3):                                            # every filter sees it
            assert bool(bad[:, f * 3:(f + 1) * 3].any()), (pad, other, f)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("side", ["above", "below"])
def test_comparator_catches_a_chunk_local_pad(pad, side):
    """an 8-row chunk [y0, y0 + 8) whose halo row y0 - 1 (or y0 + 8) is its own first (last) row: padding resolved inside the chunk"""
    shape, y0 = (1, 2, 24, 12), 8
    x = rand(shape, 320)
    got = dynca_eval(x, pad)
    sub = x[:, :, y0 - 1:y0 + 9].clone()                              # rows y0 - 1 .. y0 + 8
    if side == "above":
        sub[:, :, 0] = sub[:, :, 1]
    else:
        sub[:, :, 9] = sub[:, :, 8]
    # horizontal padding as the mode has it, vertical halo rows explicit: evaluate with the rows in place and keep the inner 8
    wrong = dynca_eval(F.pad(sub, [1, 1, 0, 0], pad) if pad != "constant" else F.pad(sub, [1, 1, 0, 0]), "constant")[:, :, 1:9, 1:-1]
    got[:, :, y0:y0 + 8] = wrong
    same, bad, worst = check_dynca(got, x, pad)
    row = y0 if side == "above" else y0 + 7
    assert same and bool(bad.any()) and worst > 1.0
    assert not bool(bad[:, :, :row].any()) and not bool(bad[:, :, row + 1:].any())     # the one row that read the halo
    assert bool(bad[:, 2:4].any()) and bool(bad[:, 4:6].any())                         # Sobel y and the Laplacian read it


def wave_edge_mask(shape, lane):
    """[B,C,H,W] bool: the cell of the one-row vector form (thread = 4 cells of a row, id = ((b C + c) H + y) W/4 + x4) that reads
    across the wave edge: column 4 x4 + 3 of a thread in lane 63 that is not the last of its row, column 4 x4 of one in lane 0 that is
    not the first"""
    B, C, H, W = shape
    W4 = W // 4
    ids = torch.arange(B * C * H * W4).reshape(B, C, H, W4)
    x4 = ids % W4
    hit = (ids % 64 == lane) & ((x4 < W4 - 1) if lane == 63 else (x4 > 0))
    m = torch.zeros(shape, dtype=torch.bool)
    m[..., (3 if lane == 63 else 0)::4] = hit
    return m


@pytest.mark.parametrize("shape", [(3, 5, 7, 36), (1, 2, 3, 260)])
@pytest.mark.parametrize("lane", [0, 63])
def test_comparator_catches_a_wrong_wave_edge_neighbour(shape, lane):
    """every 64th thread takes its right neighbour from column 4 x4 + 3 in place of 4 x4 + 4 (lane 63), or its left one from 4 x4 in
    place of 4 x4 - 1 (lane 0): the stencil with that tap column folded onto the centre column"""
    x = rand(shape, 330)
    mask = wave_edge_mask(shape, lane)
    assert bool(mask.any())                                           # W / 4 = 9 and 65 do not divide 64: such threads exist
    C = shape[1]
    for pad in PADS:
        got = dynca_eval(x, pad)
        for f, filt in enumerate(DYNCA_FILTERS, 1):
            w = _t(filt, x).clone()
            src = 2 if lane == 63 else 0
            w[:, 1] += w[:, src]
            w[:, src] = 0
            got[:, f * C:(f + 1) * C] = torch.where(mask, stencil(x, w, pad), got[:, f * C:(f + 1) * C])
        same, bad, worst = check_dynca(got, x, pad)
        assert same and bool(bad.any()) and worst > 1.0, pad
        assert not bool((bad & ~mask.repeat(1, 3, 1, 1)).any()), pad
        assert bool(bad[:, :C].any()) and bool(bad[:, 2 * C:].any()), pad      # Sobel x and the Laplacian read that column
