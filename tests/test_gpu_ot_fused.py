"""The fused relaxed-EMD kernels of the OT appearance loss (csrc/nca_ot.hip, ncahip.loss.ot_loss_fused) against a float64
evaluation of the reference's formulas (EncoderConditioning/loss/appearance_loss.py:149-220) written out here with numpy, closed-form
gradients included -- never against the kernels themselves.

Inputs are ReLU-shaped like VGG features, relu(randn + 0.3), seeded.  Argmins are compared on every row / column whose float64
best-to-second-best gap is >= GAP = 1e-5; a case in which more than 1 % of the B*N rows or of the B*N columns fall below that gap (for
B*N < 100: any at all) fails as a bad input instead of passing.  Gradients are compared on the positions fed only by rows / columns
that passed the gap test.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 1e-5
EPS = 1e-10


# ------------------------------------------------------------------------------------------------ float64 yardstick (numpy)
def feats(rng, *shape):
    return np.maximum(rng.standard_normal(shape) + 0.3, 0.0).astype(np.float32)


def ref_dist(x, y):
    """x, y [N, c] float64 -> d [N, N] (appearance_loss.py:150-156)"""
    xn = np.sqrt((x ** 2).sum(1))[:, None]
    yn = np.sqrt((y ** 2).sum(1))[None, :]
    return 1.0 - (x @ y.T) / (xn + EPS) / (yn + EPS)


def ref_remd(x, y):
    """One sample, float64: dict with d, rmin / rarg / rgap (over j, per row i), cmin / carg / cgap (over i, per column j), the two
    means, remd and the branch (0 = the row mean won)."""
    d = ref_dist(x.astype(np.float64), y.astype(np.float64))
    n = d.shape[0]
    out = {"d": d, "rmin": d.min(1), "rarg": d.argmin(1), "cmin": d.min(0), "carg": d.argmin(0)}
    if n > 1:
        s1, s0 = np.partition(d, 1, axis=1), np.partition(d, 1, axis=0)
        out["rgap"], out["cgap"] = s1[:, 1] - s1[:, 0], s0[1] - s0[0]
    else:
        out["rgap"] = out["cgap"] = np.full(n, np.inf)
    # gap between the best entry and the best entry OUTSIDE its group of identical vectors (groups: index -> lowest copy)
    def _gap(v, best, groups):
        other = np.array([groups.get(k, k) != groups.get(best, best) for k in range(v.size)])
        return (v[other].min() - v[best]) if other.any() else np.inf
    out["rgap_groups"] = lambda i, groups: _gap(d[i], out["rarg"][i], groups)
    out["cgap_groups"] = lambda j, groups: _gap(d[:, j], out["carg"][j], groups)
    out["mr"], out["mc"] = out["rmin"].mean(), out["cmin"].mean()
    out["remd"] = max(out["mr"], out["mc"])
    out["branch"] = 0 if out["mr"] > out["mc"] else 1
    return out


def ref_dd_dy(xi, yj):
    """d d_ij / d y_j in float64, norms as functions of the vectors; the 0 / 0 of the second term at y_j = 0 is taken as 0."""
    xh = xi / (np.sqrt((xi ** 2).sum()) + EPS)
    ny = np.sqrt((yj ** 2).sum())
    s = ny + EPS
    g = -xh / s
    if ny > 0:
        g = g + (xh @ yj) * yj / (ny * s * s)
    return g


def ref_remd_grad(x, y, r, up):
    """dL/dy [N, c] float64 for L = up * remd, through the float64 argmins of the winning branch; and `ok` [N]: rows of dL/dy fed only
    by rows / columns of d that passed the gap test."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    n = x.shape[0]
    g, ok = np.zeros_like(y), np.ones(n, bool)
    if r["branch"] == 1:
        for j in range(n):
            g[j] = up / n * ref_dd_dy(x[r["carg"][j]], y[j])
        ok = r["cgap"] >= GAP
    else:
        for i in range(n):
            j = r["rarg"][i]
            g[j] += up / n * ref_dd_dy(x[i], y[j])
            if r["rgap"][i] < GAP:                       # a near-tie row may land on any of its near-best columns
                ok[r["d"][i] - r["rmin"][i] < GAP] = False
    return g, ok


def check_cap(gaps, what):
    """The exclusion cap of the module docstring; returns the mask of rows that are compared."""
    keep = gaps >= GAP
    n, out = keep.size, int((~keep).sum())
    assert out <= (0 if n < 100 else 0.01 * n), f"bad input: {out} of {n} {what} have a float64 gap below {GAP}"
    return keep


def ref_moment_grad(x, y, up):
    """value [B] and d/dy of up * sum_b moment(x_b, y_b) in float64 (torch autograd on the CPU: abs and products only)"""
    xt = torch.from_numpy(x.astype(np.float64))
    yt = torch.from_numpy(y.astype(np.float64)).requires_grad_(True)
    mx, my = xt.mean(1, keepdim=True), yt.mean(1, keepdim=True)
    xc, yc = xt - mx, yt - my
    n = xt.shape[1]
    cx, cy = torch.bmm(xc.transpose(1, 2), xc) / (n - 1), torch.bmm(yc.transpose(1, 2), yc) / (n - 1)
    mom = (mx - my).abs().mean(dim=(1, 2)) + (cx - cy).abs().mean(dim=(1, 2))
    (mom.sum() * up).backward()
    return mom.detach().numpy(), yt.grad.numpy()


def ref_ot_layer(t, g, up=None):
    """One style layer with every position used (h <= 32): t [1,c,h,w], g [B,c,h,w] float32 arrays -> float64 loss value
    (ot_loss_* semantics: batch mean of remd + moment), dL/dg [B,c,h,w], the mask of comparable positions [B,h*w], and the
    per-sample records."""
    B, c, h, w = g.shape
    up = 1.0 / B if up is None else up
    x = np.broadcast_to(t.reshape(1, c, h * w).transpose(0, 2, 1), (B, h * w, c))
    y = g.reshape(B, c, h * w).transpose(0, 2, 1)
    recs = [ref_remd(x[b], y[b]) for b in range(B)]
    mom, gy = ref_moment_grad(x, y, up)
    ok = np.ones((B, h * w), bool)
    for b in range(B):
        gb, ok[b] = ref_remd_grad(x[b], y[b], recs[b], up)
        gy[b] += gb
    val = up * sum(r["remd"] for r in recs) + up * mom.sum()
    return val, gy.transpose(0, 2, 1).reshape(B, c, h, w), ok, recs


def branch_inputs(seed, branch, c=64, hw=32, B=2, anchors=8, noise=0.1):
    """Maps whose relaxed EMD takes the wanted branch by construction.  branch 0 (the row mean wins): every generated vector is a
    small perturbation of one of a handful of target vectors, so every column has a near neighbour (small column mean) while most
    target rows have none (large row mean).  branch 1: the mirror image, the target's vectors cluster around a handful of generated
    ones."""
    rng = np.random.default_rng(seed)
    n = hw * hw
    free = feats(rng, B, n, c)                                            # per sample: the side that keeps independent vectors
    pick = rng.integers(0, anchors, size=(B, n))
    if branch == 0:                                                       # target free (one map for the batch), generated clustered
        x = free[0]
        y = np.maximum(x[pick] + noise * rng.standard_normal((B, n, c)), 0.0).astype(np.float32)
    else:                                                                 # generated free; the target clusters around sample 0's anchors
        y = free
        y[1:, :anchors] = y[0, :anchors]                                  # every sample holds the anchors
        x = np.maximum(y[0][pick[0]] + noise * rng.standard_normal((n, c)), 0.0).astype(np.float32)
    t = np.ascontiguousarray(x.T.reshape(1, c, hw, hw))
    g = np.ascontiguousarray(y.transpose(0, 2, 1).reshape(B, c, hw, hw))
    return t, g


def grad_errors(got, ref, ok):
    """(relative L2, max-abs / largest entry) of dL/dg [B,c,h,w] on the positions ok [B,h*w]"""
    B, c = ref.shape[:2]
    m = np.broadcast_to(ok[:, None, :], (B, c, ok.shape[1])).reshape(ref.shape)
    d = (got.astype(np.float64) - ref)[m]
    return float(np.linalg.norm(d) / np.linalg.norm(ref[m])), float(np.abs(d).max() / np.abs(ref[m]).max())


def torch_cpu_fp32_grad(t, g):
    """dL/dg of ot_loss_batched in plain fp32 torch on the CPU: the measurement the gradient bounds stand on."""
    from ncahip.loss import ot_loss_batched
    gt = torch.from_numpy(g).requires_grad_(True)
    ot_loss_batched([torch.from_numpy(t)], [gt]).backward()
    return gt.grad.numpy()


# ------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("c,h,w,B,sampled", [(64, 40, 40, 3, True), (512, 16, 16, 2, False), (12, 7, 9, 2, True), (128, 34, 33, 2, True),
                                              (256, 2, 2, 3, False)])
def test_gather_matches_torch_and_its_adjoint(c, h, w, B, sampled):
    from ncahip import ops
    rng = np.random.default_rng(c + h)
    t, g = torch.from_numpy(feats(rng, 1, c, h, w)).to(DEV), torch.from_numpy(feats(rng, B, c, h, w)).to(DEV)
    N = min(1000, (h * w) * 5 // 8) if sampled else h * w
    ix = None
    if sampled:
        ix = torch.from_numpy(np.stack([np.sort(rng.choice(h * w, N, replace=False)) for _ in range(B)]).astype(np.int32)).to(DEV)
    x, y, xn, yn = ops.ot_gather(t, g, ix)
    tv, gv = t.reshape(1, c, -1).expand(B, c, -1), g.reshape(B, c, -1)
    if sampled:
        e = ix.long()[:, None, :].expand(B, c, N)
        tv, gv = tv.gather(2, e), gv.gather(2, e)
    assert torch.equal(x, tv.transpose(1, 2).contiguous()) and torch.equal(y, gv.transpose(1, 2).contiguous())
    for got, v in ((xn, x), (yn, y)):
        ref = v.double().cpu().pow(2).sum(2).sqrt()
        err = float(((got.double().cpu() - ref).abs() / ref.clamp_min(1e-30)).max())
        print(f"gather c={c} N={N}: worst relative norm error {err:.2e}")
        assert err <= 1e-6
    dy = torch.from_numpy(rng.standard_normal((B, N, c)).astype(np.float32)).to(DEV)
    dg = ops.ot_gather_backward(dy, ix, h, w)
    ref = torch.zeros(B, c, h * w, device=DEV)
    if sampled:
        for b in range(B):
            ref[b].index_add_(1, ix[b].long(), dy[b].t().contiguous())
    else:
        ref = dy.transpose(1, 2).contiguous()
    assert torch.equal(dg.reshape(B, c, -1), ref)
    ops.check_errors()


# ------------------------------------------------------------------------------------------------------------------ forward
def run_remd(x, y):
    from ncahip import ops
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    B, N, c = xt.shape
    xn, yn = xt.pow(2).sum(2).sqrt(), yt.pow(2).sum(2).sqrt()
    r = ops.ot_remd(xt, yt, xn, yn)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}, (xt, yt, xn, yn)


@pytest.mark.parametrize("c,N,B", [(64, 1000, 3), (128, 1000, 2), (256, 1000, 2), (512, 1000, 2), (512, 1024, 2), (512, 256, 4),
                                   (512, 16, 8), (512, 4, 8), (12, 37, 3)])
def test_forward_against_float64(c, N, B):
    rng = np.random.default_rng(1000 * c + N)
    x, y = feats(rng, B, N, c), feats(rng, B, N, c)
    assert (x.any(2) & y.any(2)).all()                                    # zero vectors have a case of their own
    got, _ = run_remd(x, y)
    recs = [ref_remd(x[b], y[b]) for b in range(B)]
    rkeep = check_cap(np.stack([r["rgap"] for r in recs]), "rows")
    ckeep = check_cap(np.stack([r["cgap"] for r in recs]), "columns")
    for k in ("rmin", "cmin"):
        err = float(np.abs(got[k] - np.stack([r[k] for r in recs])).max())
        print(f"forward c={c} N={N} B={B}: {k} worst abs error {err:.2e}")
        assert err <= 2e-6, (k, err)
    remd = np.array([r["remd"] for r in recs])
    err = float((np.abs(got["remd"] - remd) / remd).max())
    print(f"forward c={c} N={N} B={B}: remd worst relative error {err:.2e}; rows left out {int((~rkeep).sum())}, columns {int((~ckeep).sum())}")
    assert err <= 1e-6
    assert (got["rarg"] == np.stack([r["rarg"] for r in recs]))[rkeep].all()
    assert (got["carg"] == np.stack([r["carg"] for r in recs]))[ckeep].all()
    for b, r in enumerate(recs):
        if abs(r["mr"] - r["mc"]) > 1e-6:
            assert got["branch"][b] == r["branch"]


def test_exact_ties_take_the_lowest_index_and_runs_are_bit_identical():
    """Duplicated feature vectors on both sides: d has exactly equal entries, within a tile, across tiles of one workgroup and
    across workgroups.  A row whose nearest column is duplicated must report the lowest copy, and likewise for columns."""
    rng = np.random.default_rng(7)
    B, N, c = 2, 1000, 64
    x, y = feats(rng, B, N, c), feats(rng, B, N, c)
    ydup = {3: (3, 17, 40, 70, 333, 999), 500: (500, 777), 64: (64, 65)}        # lowest copy -> all copies
    xdup = {5: (5, 6, 63, 64, 129, 640, 998), 200: (200, 900)}
    for lo, cps in ydup.items():
        y[:, list(cps)] = y[:, lo:lo + 1]
    for lo, cps in xdup.items():
        x[:, list(cps)] = x[:, lo:lo + 1]
    # make the duplicated vectors somebody's nearest neighbour: rows 10..13 are near y[3], columns 20..23 near x[5]
    x[:, 10:14] = np.maximum(y[:, 3:4] + 0.02 * rng.standard_normal((B, 4, c)), 0).astype(np.float32)
    y[:, 20:24] = np.maximum(x[:, 5:6] + 0.02 * rng.standard_normal((B, 4, c)), 0).astype(np.float32)
    got, _ = run_remd(x, y)
    again, _ = run_remd(x, y)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    ycopies = {j: lo for lo, cps in ydup.items() for j in cps}
    xcopies = {i: lo for lo, cps in xdup.items() for i in cps}
    for b in range(B):
        # the float64 products of two copies need not agree to the last bit (a library matrix product may sum them in different
        # orders), so the yardstick names the GROUP of the nearest neighbour and the expectation is that group's lowest member
        r = ref_remd(x[b], y[b])
        assert all(ycopies.get(r["rarg"][i]) == 3 for i in range(10, 14)) and all(xcopies.get(r["carg"][j]) == 5 for j in range(20, 24))
        hit = 0
        for i in range(N):
            if r["rarg"][i] in ycopies and r["rgap_groups"](i, ycopies) >= GAP:
                assert got["rarg"][b, i] == ycopies[r["rarg"][i]], (b, i)
                hit += 1
        for j in range(N):
            if r["carg"][j] in xcopies and r["cgap_groups"](j, xcopies) >= GAP:
                assert got["carg"][b, j] == xcopies[r["carg"][j]], (b, j)
                hit += 1
        assert hit >= 8
        # equal vectors give bit-equal distances: the copies' own minima agree exactly
        for lo, cps in ydup.items():
            assert len({got["cmin"][b, j].tobytes() for j in cps}) == 1 and len({int(got["carg"][b, j]) for j in cps}) == 1
        for lo, cps in xdup.items():
            assert len({got["rmin"][b, i].tobytes() for i in cps}) == 1 and len({int(got["rarg"][b, i]) for i in cps}) == 1


# ----------------------------------------------------------------------------------------------------------------- backward
def fused_grad(t, g, seed=None):
    from ncahip.loss import ot_loss_fused
    gt = torch.from_numpy(g).to(DEV).requires_grad_(True)
    if seed is not None:
        np.random.seed(seed)
    val = ot_loss_fused([torch.from_numpy(t).to(DEV)], [gt])
    val.backward()
    return float(val), gt.grad.cpu().numpy()


# plain fp32 torch on the CPU against the float64 yardstick, same inputs, same positions (measured while writing this test, see
# each case's figures in test_backward_against_float64's docstring): the bound is 10 x that figure or 1e-5, whichever is larger
BWD_CASES = [  # (name, maker, wanted branch)
    ("rows c=64", lambda: branch_inputs(11, 0), 0),
    ("columns c=64", lambda: branch_inputs(12, 1), 1),
    ("rows c=512 N=256", lambda: branch_inputs(13, 0, c=512, hw=16, B=3), 0),
    ("columns c=128 N=1024", lambda: branch_inputs(14, 1, c=128, hw=32, B=2), 1),
]


@pytest.mark.parametrize("name,make,branch", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_against_float64(name, make, branch):
    """dL/dG of ot_loss_fused (relaxed EMD through the kernels + moment term on the gathered X, Y + the scatter) against the float64
    gradient of the same formulas, on the positions fed only by rows / columns that passed the gap test.

    Plain fp32 torch (ot_loss_batched on the CPU) against the same yardstick on the same positions, measured when these seeds
    were fixed -- (relative L2, max-abs / largest entry):
        rows c=64              (1.1e-07, 1.8e-07)
        columns c=64           (7.9e-08, 2.0e-07)
        rows c=512 N=256       (1.0e-07, 2.8e-07)
        columns c=128 N=1024   (8.6e-08, 2.2e-07)
    10 x those figures is below 1e-5 everywhere, so the bound is 1e-5 for both measures.  The kernels, measured on an MI355X with
    these seeds: rel L2 6.8e-08 .. 1.3e-07, max-abs / max 1.5e-07 .. 3.5e-07."""
    t, g = make()
    val, ref, ok, recs = ref_ot_layer(t, g)
    for r in recs:
        assert r["branch"] == branch and abs(r["mr"] - r["mc"]) > 1e-4, (r["mr"], r["mc"])     # no near-tie of the outer max
    check_cap(np.stack([r["rgap"] for r in recs]), "rows")
    check_cap(np.stack([r["cgap"] for r in recs]), "columns")
    assert ok.mean() > 0.95
    got_val, got = fused_grad(t, g)
    assert np.isfinite(got).all()
    l2, mx = grad_errors(got, ref, ok)
    print(f"backward {name}: value rel err {abs(got_val - val) / val:.2e}, gradient rel L2 {l2:.2e}, max-abs / max {mx:.2e}, "
          f"positions compared {ok.mean():.4f}")
    assert abs(got_val - val) <= 1e-5 * val
    assert l2 <= 1e-5 and mx <= 1e-5


def test_zero_vectors_give_finite_gradients():
    """Three all-zero generated vectors and three all-zero target vectors (N = 1024).  The torch path returns NaN gradients when a
    zero generated vector sits on the winning branch (0 / 0 in the backward of sqrt); the fused path returns the finite closed
    form with the zero vectors' own second term taken as 0, and agrees with the float64 closed form everywhere else.  The zero
    vectors tie exactly against everything (d = 1), so their rows / columns fail the gap test and are left out of the
    comparison by the same rule as any other near-tie; they are still checked to be finite."""
    t, g = branch_inputs(21, 1, c=64, hw=32, B=2)                          # column branch: every generated vector receives a pair
    zy, zx = (100, 517, 1023), (7, 300, 800)
    g.reshape(2, 64, -1)[:, :, list(zy)] = 0.0
    t.reshape(1, 64, -1)[:, :, list(zx)] = 0.0
    val, ref, ok, recs = ref_ot_layer(t, g)
    for r in recs:
        assert r["branch"] == 1 and abs(r["mr"] - r["mc"]) > 1e-4
        assert (~(r["cgap"] >= GAP)).sum() <= 0.01 * r["cgap"].size + len(zy)
    assert not ok[:, list(zy)].any()                                        # d = 1 against everything: an exact tie
    from ncahip.loss import ot_loss_batched
    gt = torch.from_numpy(g).to(DEV).requires_grad_(True)
    ot_loss_batched([torch.from_numpy(t).to(DEV)], [gt]).backward()
    assert not bool(torch.isfinite(gt.grad).all())                          # what the torch path does there
    got_val, got = fused_grad(t, g)
    assert np.isfinite(got).all() and np.isfinite(got_val)
    l2, mx = grad_errors(got, ref, ok)
    print(f"zero vectors: gradient rel L2 {l2:.2e}, max-abs / max {mx:.2e}")
    assert l2 <= 1e-5 and mx <= 1e-5
    # the zero generated vectors themselves: -xh / s from the pair (carg = lowest index: row 0) + the moment term, second term 0
    B, c = g.shape[:2]
    for b in range(B):
        for j in zy:
            want = ref[b].reshape(c, -1)[:, j]                              # closed form with carg = argmin's first minimum = 0
            assert recs[b]["carg"][j] == 0
            have = got[b].reshape(c, -1)[:, j]
            assert np.abs(have - want).max() <= 1e-5 * np.abs(want).max()
            assert np.abs(want).max() > 1e3                                 # 1 / (0 + 1e-10): large, finite


# ---------------------------------------------------------------------------------------------------- against the parent's path
def test_fused_equals_batched_on_the_same_draws():
    from ncahip.loss import ot_loss_batched, ot_loss_fused
    rng = np.random.default_rng(5)
    B = 3
    shapes = [(64, 48, 48), (128, 40, 40), (256, 32, 32), (512, 16, 16), (512, 8, 8)]
    tf = [torch.from_numpy(feats(rng, 1, *s)).to(DEV) for s in shapes]
    gf = [torch.from_numpy(feats(rng, B, *s)).to(DEV) for s in shapes]
    np.random.seed(123)
    a = ot_loss_batched(tf, gf)
    sa = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(123)
    b = ot_loss_fused(tf, gf)
    sb = np.random.get_state()[1].copy(), np.random.get_state()[2]
    assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1]                  # the numpy stream is left at the same position
    rel = abs(float(a) - float(b)) / abs(float(a))
    print(f"fused vs batched, five layers: {float(a):.8f} vs {float(b):.8f}, rel {rel:.2e}")
    assert rel <= 1e-5


def test_loss_module_fused_equals_default_end_to_end():
    """Loss(ot_impl='fused') vs Loss() through the seeded-random VGG at 4 x 3 x 128^2: loss within 1e-5 relative, dL/d(generated
    image) relative L2 <= 1e-4 (a flipped near-tie argmin is amplified through the VGG backward, hence looser than the kernel-level
    bound).  Measured on an MI355X: loss equal to the last printed digit, image-gradient relative L2 2.4e-05."""
    from ncahip.loss import Loss
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(128, 128, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        La, Lb = Loss(dev, target_style_image=style), Loss(dev, target_style_image=style, ot_impl="fused")
    gen0 = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(1))
    out = []
    for L in (La, Lb):
        gen = gen0.to(dev).requires_grad_(True)
        d = {"generated_images": gen, "nca_state": torch.rand(4, 16, 128, 128, generator=torch.Generator().manual_seed(2)).to(dev) * 3 - 1.5,
             "target_images": torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(3)).to(dev)}
        np.random.seed(9)
        loss, log = L(d)
        loss.backward()
        out.append((float(loss), gen.grad.double().cpu(), float(log["appearance"]), np.random.get_state()[2]))
    (la, ga, aa, pa), (lb, gb, ab, pb) = out
    rel, l2 = abs(la - lb) / abs(la), float((ga - gb).norm() / ga.norm())
    print(f"Loss end to end: loss {la:.8f} vs {lb:.8f} (rel {rel:.2e}), appearance {aa:.8f} vs {ab:.8f}, image-gradient rel L2 {l2:.2e}")
    assert pa == pb
    assert rel <= 1e-5
    assert l2 <= 1e-4


# -------------------------------------------------------------------------------------------------------------- determinism
def test_forward_and_backward_are_bit_reproducible():
    t, g = branch_inputs(31, 0, c=128, hw=32, B=2)
    t2, g2 = branch_inputs(32, 1, c=64, hw=32, B=2)
    for tt, gg in ((t, g), (t2, g2)):
        a, b = fused_grad(tt, gg), fused_grad(tt, gg)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    rng = np.random.default_rng(3)
    tm, gm = feats(rng, 1, 64, 40, 40), feats(rng, 2, 64, 40, 40)          # the sampled path
    a, b = fused_grad(tm, gm, seed=4), fused_grad(tm, gm, seed=4)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_runs_with_the_fused_loss():
    import random
    from ncahip import ops
    from ncahip.conditioned_trainer import ConditionedNCATrainer
    from ncahip.loss import Loss
    from ncahip.nca import ConditionedNCA

    class DS(torch.utils.data.Dataset):
        target_size = (3, 64, 64)

        def __init__(self):
            self.x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(0))

        def __len__(self):
            return 8

        def __getitem__(self, i):
            return self.x[i]

    dev = torch.device(DEV)
    torch.manual_seed(3)
    m = ConditionedNCA(target_shape=(3, 64, 64)).to(dev)
    style = (np.random.RandomState(0).rand(64, 64, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        L = Loss(dev, target_style_image=style, ot_impl="fused")
    tr = ConditionedNCATrainer(m, DS(), None, nca_steps=[4, 8], lr=2e-3, pool_size=16, log_base_path="/tmp/ncahip_gpu_test",
                               loss=L, device=dev)
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    losses = []
    orig = tr.train_batch
    tr.train_batch = lambda b, t: (lambda r: (losses.append(r[1]), r)[1])(orig(b, t))
    tr.train(batch_size=4, epochs=1)
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    ops.check_errors()
