"""The fused moment-matching kernels of the OT appearance loss (csrc/nca_ot_moment.hip, ncahip.loss.ot_loss_fused_all) against a
float64 evaluation of the reference's formulas (EncoderConditioning/loss/appearance_loss.py:149-220), written out here with numpy
and CPU torch in float64 (the gradient of the moment term by float64 autograd, not by the kernels' closed form) -- never against
the kernels themselves.

Inputs are ReLU-shaped like VGG features, relu(randn + 0.3), seeded.  The sign-gap rule: an entry of D = Cx - Cy with float64
|D_kl| < SIGN_GAP = 1e-6 is a near-tie; its sign is not compared, and channels k and l of that sample are left out of the gradient
comparison.  A case in which more than 0.1 % of a sample's c^2 entries are near-ties (for c^2 < 1000: any at all), or in which more
than 10 % of a sample's channels are thereby left out, fails as a bad input instead of passing.  Positions of the gradient are
compared under test_gpu_ot_fused's argmin gap rule.  The relaxed-EMD yardstick and the gap rule are that module's helpers.
"""
import warnings

import numpy as np
import pytest
import torch

from test_gpu_ot_fused import branch_inputs, check_cap, feats, ref_remd, ref_remd_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIGN_GAP = 1e-6


# ------------------------------------------------------------------------------------------------ float64 yardstick
def ref_moment(x, y, up=1.0):
    """One sample, x, y [N, c]: dict with mom, D [c, c], the near-tie mask of D, the channels kept by the sign-gap rule, mx - my,
    and grad = d (up * mom) / d y [N, c] -- all float64; the gradient by torch autograd on the reference's formulas."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))
    yt = torch.from_numpy(np.asarray(y, dtype=np.float64)).requires_grad_(True)
    n = xt.shape[0]
    mx, my = xt.mean(0, keepdim=True), yt.mean(0, keepdim=True)
    xc, yc = xt - mx, yt - my
    d = torch.mm(xc.t(), xc) / (n - 1) - torch.mm(yc.t(), yc) / (n - 1)
    mom = (mx - my).abs().mean() + d.abs().mean()
    (mom * up).backward()
    D = d.detach().numpy()
    near = np.abs(D) < SIGN_GAP
    return {"mom": float(mom.detach()), "D": D, "near": near, "keep": ~(near.any(0) | near.any(1)), "dm": (mx - my).detach().numpy()[0],
            "grad": yt.grad.numpy()}


def check_sign_caps(m, what):
    """The two caps of the module docstring on one sample's record; returns (near-tie entries, channels left out)."""
    c = m["D"].shape[0]
    nn, nc = int(m["near"].sum()), int((~m["keep"]).sum())
    assert nn <= (0 if c * c < 1000 else 0.001 * c * c), f"bad input ({what}): {nn} of {c * c} entries of D are near-ties"
    assert nc <= 0.1 * c, f"bad input ({what}): {nc} of {c} channels left out"
    return nn, nc


def ref_layer(t, g, idx=None):
    """One style layer, t [1,c,h,w], g [B,c,h,w] float32 arrays, idx [B,N] sampled positions or None (every position): float64 value
    of ot_loss_* (batch mean of relaxed EMD + moment term), dL/dg [B,c,h,w], the mask of comparable positions [B,h*w] (argmin gap
    rule), the mask of comparable channels [B,c] (sign-gap rule), and the per-sample records."""
    B, c, h, w = g.shape
    hw, up = h * w, 1.0 / B
    tv, gv = t.reshape(c, hw).T, g.reshape(B, c, hw).transpose(0, 2, 1)
    val, dg = 0.0, np.zeros((B, hw, c))
    okpos, keepch, recs, moms = np.zeros((B, hw), bool), np.ones((B, c), bool), [], []
    for b in range(B):
        ix = np.arange(hw) if idx is None else idx[b]
        x, y = tv[ix], gv[b][ix]
        r = ref_remd(x, y)
        gr, ok = ref_remd_grad(x, y, r, up)
        m = ref_moment(x, y, up)
        val += up * (r["remd"] + m["mom"])
        dg[b, ix] = gr + m["grad"]
        okpos[b, ix], keepch[b] = ok, m["keep"]
        recs.append(r)
        moms.append(m)
    return val, dg.transpose(0, 2, 1).reshape(B, c, h, w), okpos, keepch, recs, moms


def draw_idx(seed, B, hw, n_samples=1000):
    """The draws ot_loss_* make for one sampled layer after np.random.seed(seed)"""
    np.random.seed(seed)
    return np.stack([np.sort(np.random.choice(np.arange(hw), size=n_samples, replace=False)) for _ in range(B)])


def masked_grad_errors(got, ref, okpos, keepch):
    """(relative L2, max-abs / largest entry) of dL/dg [B,c,h,w] on positions okpos [B,h*w] x channels keepch [B,c]"""
    m = (keepch[:, :, None] & okpos[:, None, :]).reshape(ref.shape)
    d = (np.asarray(got, dtype=np.float64) - ref)[m]
    return float(np.linalg.norm(d) / np.linalg.norm(ref[m])), float(np.abs(d).max() / np.abs(ref[m]).max())


# ------------------------------------------------------------------------------------------------------------------ forward
FWD_CASES = [(12, 2, 2, 30), (12, 37, 3, 1), (64, 37, 8, 2), (64, 1000, 3, 3), (128, 1024, 2, 4), (256, 256, 4, 5), (512, 1000, 2, 6),
             (512, 1024, 2, 7)]   # (c, N, B, seed)


def fwd_inputs(c, N, B, seed):
    rng = np.random.default_rng(seed)
    return feats(rng, B, N, c), feats(rng, B, N, c)


@pytest.mark.parametrize("c,N,B,seed", FWD_CASES)
def test_forward_against_float64(c, N, B, seed):
    """mom [B] and S = sign(Cx - Cy) of ops.ot_moment against float64.

    Plain fp32 torch on the CPU (ncahip.loss._moment_loss per sample) against the same yardstick on the same inputs, worst relative
    error of mom over the batch, measured when these seeds were fixed:
        c=12 N=2 4.3e-08   c=12 N=37 8.0e-08   c=64 N=37 8.3e-08   c=64 N=1000 1.3e-07   c=128 N=1024 1.5e-07
        c=256 N=256 1.0e-07   c=512 N=1000 4.2e-08   c=512 N=1024 5.0e-08
    10 x those figures is below 1e-5 everywhere, so the bound is 1e-5 (relative) for every case.  (Two ReLU rows share their zeros,
    so at N = 2 about 8 % of a typical D is exactly zero, a tie by construction; the N = 2 seed is one whose D has no zero.)
    The kernels, measured on an MI355X with these seeds, in the same order: 4.3e-08, 8.0e-08, 6.2e-08, 1.9e-07, 1.0e-07, 7.9e-08,
    4.9e-08, 9.2e-08; every compared sign equal; near-tie entries per sample 0 up to c = 128, at most 4 at c = 256, 18 at c = 512."""
    from ncahip import ops
    x, y = fwd_inputs(c, N, B, seed)
    recs = [ref_moment(x[b], y[b]) for b in range(B)]
    left = [check_sign_caps(m, f"sample {b}") for b, m in enumerate(recs)]
    assert all(np.abs(m["dm"]).min() >= SIGN_GAP for m in recs)              # no near-tie among the mean differences either
    got = ops.ot_moment(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    torch.cuda.synchronize()
    mom, S, sgn = got["mom"].cpu().numpy(), got["S"].cpu().numpy(), got["sgn"].cpu().numpy()
    ref = np.array([m["mom"] for m in recs])
    err = float((np.abs(mom - ref) / ref).max())
    print(f"forward c={c} N={N} B={B}: mom worst relative error {err:.2e}; near-tie entries / channels left out per sample {left}")
    assert err <= 1e-5
    assert set(np.unique(S)) <= {-1, 0, 1}
    for b, m in enumerate(recs):
        assert np.array_equal(S[b][~m["near"]], np.sign(m["D"]).astype(np.int8)[~m["near"]]), b
        assert np.array_equal(S[b], S[b].T)
        assert np.array_equal(sgn[b], np.sign(m["dm"]).astype(np.float32))
    ym = got["my"].cpu().numpy().astype(np.float64)
    assert np.abs(ym - y.astype(np.float64).mean(1)).max() <= 1e-6
    ops.check_errors()


# ----------------------------------------------------------------------------------------------------------------- backward
def fused_all_grad(t, g, seed=None):
    from ncahip.loss import ot_loss_fused_all
    gt = torch.from_numpy(g).to(DEV).requires_grad_(True)
    if seed is not None:
        np.random.seed(seed)
    val = ot_loss_fused_all([torch.from_numpy(t).to(DEV)], [gt])
    val.backward()
    return float(val.detach()), gt.grad.cpu().numpy()


BWD_CASES = [  # (name, maker of (t, g), wanted branch, seed of the index draws or None for an un-sampled layer)
    ("rows c=64 N=1024", lambda: branch_inputs(11, 0), 0, None),
    ("columns c=128 N=1024", lambda: branch_inputs(14, 1, c=128, hw=32, B=2), 1, None),
    ("rows c=512 N=256", lambda: branch_inputs(13, 0, c=512, hw=16, B=3), 0, None),
    ("columns c=12 N=64", lambda: branch_inputs(15, 1, c=12, hw=8, B=8), 1, None),
    ("sampled rows c=64 40x40", lambda: branch_inputs(16, 0, c=64, hw=40, B=3), 0, 21),
    ("sampled columns c=256 36x36", lambda: branch_inputs(17, 1, c=256, hw=36, B=2), 1, 22),
]


@pytest.mark.parametrize("name,make,branch,seed", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_backward_against_float64(name, make, branch, seed):
    """dL/dG of ot_loss_fused_all (gather, relaxed EMD, moment term, one dY, one scatter: all kernels) against the float64 gradient
    of the same formulas, on the positions that pass the argmin gap rule and the channels that pass the sign-gap rule.

    Plain fp32 torch (ot_loss_batched on the CPU, same index draws) against the same yardstick on the same positions and channels,
    measured when these seeds were fixed -- (value relative error, gradient relative L2, max-abs / largest entry):
        rows c=64 N=1024              (9.9e-08, 1.1e-07, 1.8e-07)
        columns c=128 N=1024          (8.4e-09, 8.6e-08, 2.2e-07)
        rows c=512 N=256              (3.5e-08, 1.0e-07, 2.8e-07)
        columns c=12 N=64             (3.6e-08, 9.7e-08, 1.2e-07)
        sampled rows c=64 40x40       (4.6e-09, 1.0e-07, 1.8e-07)
        sampled columns c=256 36x36   (6.6e-09, 1.1e-07, 2.5e-07)
    10 x those figures is below 1e-5 everywhere, so the bound is 1e-5 for all three measures.  The kernels, measured on an MI355X
    with these seeds, in the same order: (7.4e-08, 8.8e-08, 3.0e-07), (8.4e-09, 6.8e-08, 1.6e-07), (3.8e-08, 1.2e-07, 2.9e-07),
    (3.6e-08, 8.1e-08, 1.1e-07), (7.6e-08, 8.5e-08, 1.5e-07), (6.6e-09, 8.3e-08, 1.8e-07); channels left out: at most 6 of 512."""
    t, g = make()
    B, c, h, w = g.shape
    idx = None if seed is None else draw_idx(seed, B, h * w)
    val, ref, okpos, keepch, recs, moms = ref_layer(t, g, idx)
    for r in recs:
        assert r["branch"] == branch and abs(r["mr"] - r["mc"]) > 1e-4, (r["mr"], r["mc"])     # no near-tie of the outer max
    check_cap(np.stack([r["rgap"] for r in recs]), "rows")
    check_cap(np.stack([r["cgap"] for r in recs]), "columns")
    left = [check_sign_caps(m, f"sample {b}") for b, m in enumerate(moms)]
    sampled = okpos if idx is None else np.stack([np.isin(np.arange(h * w), idx[b]) for b in range(B)])
    assert okpos.sum() > 0.95 * sampled.sum()
    got_val, got = fused_all_grad(t, g, seed)
    assert np.isfinite(got).all()
    if idx is not None:
        assert not got.reshape(B, c, -1).transpose(0, 2, 1)[~sampled].any()                     # nothing outside the sampled positions
    l2, mx = masked_grad_errors(got, ref, okpos, keepch)
    print(f"backward {name}: value rel err {abs(got_val - val) / val:.2e}, gradient rel L2 {l2:.2e}, max-abs / max {mx:.2e}, "
          f"positions compared {okpos.sum() / sampled.sum():.4f}, near-tie entries / channels left out per sample {left}")
    assert abs(got_val - val) <= 1e-5 * val
    assert l2 <= 1e-5 and mx <= 1e-5


def test_moment_backward_accumulates_into_dy():
    """ops.ot_moment_backward adds to the buffer it is given (what ot_remd_backward wrote): started from zeros it gives the
    gradient itself, v (0 + v is exact), checked against float64 under the bound of test_backward_against_float64; started from a
    base it must give fl(base + v) to the bit, since each element is one fp32 add by its one owner.  c and N are not multiples
    of 64."""
    from ncahip import ops
    rng = np.random.default_rng(9)
    B, N, c = 3, 300, 132
    x, y = feats(rng, B, N, c), feats(rng, B, N, c)
    base = (1e-6 * rng.standard_normal((B, N, c))).astype(np.float32)
    up = rng.uniform(0.5, 2.0, B).astype(np.float32)
    recs = [ref_moment(x[b], y[b], float(up[b])) for b in range(B)]
    left = [check_sign_caps(m, f"sample {b}") for b, m in enumerate(recs)]
    yt = torch.from_numpy(y).to(DEV)
    f = ops.ot_moment(torch.from_numpy(x).to(DEV), yt)
    gup = torch.from_numpy(up).to(DEV)
    v = ops.ot_moment_backward(yt, f["my"], f["sgn"], f["S"], gup).cpu().numpy()
    dy = torch.from_numpy(base).to(DEV)
    out = ops.ot_moment_backward(yt, f["my"], f["sgn"], f["S"], gup, dy)
    assert out.data_ptr() == dy.data_ptr()
    assert np.array_equal(dy.cpu().numpy(), base + v)
    for b, m in enumerate(recs):
        k = m["keep"]
        d = v[b][:, k].astype(np.float64) - m["grad"][:, k]
        l2, mx = np.linalg.norm(d) / np.linalg.norm(m["grad"][:, k]), np.abs(d).max() / np.abs(m["grad"][:, k]).max()
        print(f"moment backward alone, sample {b}: rel L2 {l2:.2e}, max-abs / max {mx:.2e}; near-tie entries / channels left out {left[b]}")
        assert l2 <= 1e-5 and mx <= 1e-5
    ops.check_errors()


# ---------------------------------------------------------------------------------------------------- against the parent's path
def test_fused_all_equals_batched_on_the_same_draws():
    from ncahip.loss import ot_loss_batched, ot_loss_fused_all
    rng = np.random.default_rng(5)
    B = 3
    shapes = [(64, 48, 48), (128, 40, 40), (256, 32, 32), (512, 16, 16), (512, 8, 8)]
    tf = [torch.from_numpy(feats(rng, 1, *s)).to(DEV) for s in shapes]
    gf = [torch.from_numpy(feats(rng, B, *s)).to(DEV) for s in shapes]
    np.random.seed(123)
    a = ot_loss_batched(tf, gf)
    sa = np.random.get_state()[1].copy(), np.random.get_state()[2]
    np.random.seed(123)
    b = ot_loss_fused_all(tf, gf)
    sb = np.random.get_state()[1].copy(), np.random.get_state()[2]
    assert np.array_equal(sa[0], sb[0]) and sa[1] == sb[1]                  # the numpy stream is left at the same position
    rel = abs(float(a) - float(b)) / abs(float(a))
    print(f"fused_all vs batched, five layers: {float(a):.8f} vs {float(b):.8f}, rel {rel:.2e}")
    assert rel <= 1e-5


def test_loss_module_fused_all_equals_default_end_to_end():
    """Loss(ot_impl='fused_all') vs Loss() through the seeded-random VGG at 4 x 3 x 128^2: loss within 1e-5 relative, dL/d(generated
    image) relative L2 <= 1e-4 (a flipped near-tie argmin or sign is amplified through the VGG backward, hence looser than the
    kernel-level bound), numpy stream position equal.  Measured on an MI355X: loss equal to the last printed digit, image-gradient
    relative L2 1.0e-06."""
    from ncahip.loss import Loss
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(128, 128, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        La, Lb = Loss(dev, target_style_image=style), Loss(dev, target_style_image=style, ot_impl="fused_all")
    assert Lb.ot_impl == "fused_all"
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


# ---------------------------------------------------------------------------------------------------------------- structure
def test_no_torch_matrix_product_in_the_fused_all_path(monkeypatch):
    t, g = branch_inputs(31, 0, c=128, hw=32, B=2)
    rng = np.random.default_rng(3)
    tm, gm = feats(rng, 1, 64, 40, 40), feats(rng, 2, 64, 40, 40)
    want = fused_all_grad(t, g), fused_all_grad(tm, gm, seed=4)

    def refuse(*a, **k):
        raise AssertionError("torch matrix product called inside ot_loss_fused_all")
    for name in ("bmm", "matmul", "mm"):
        monkeypatch.setattr(torch, name, refuse)
    got = fused_all_grad(t, g), fused_all_grad(tm, gm, seed=4)
    for a, b in zip(want, got):
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


# -------------------------------------------------------------------------------------------------------------- determinism
def test_forward_and_backward_are_bit_reproducible():
    t, g = branch_inputs(31, 0, c=128, hw=32, B=2)
    t2, g2 = branch_inputs(32, 1, c=512, hw=16, B=2)
    for tt, gg in ((t, g), (t2, g2)):
        a, b = fused_all_grad(tt, gg), fused_all_grad(tt, gg)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])
    rng = np.random.default_rng(3)
    tm, gm = feats(rng, 1, 64, 40, 40), feats(rng, 2, 64, 40, 40)          # the sampled path
    a, b = fused_all_grad(tm, gm, seed=4), fused_all_grad(tm, gm, seed=4)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_runs_with_the_fused_all_loss():
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
        L = Loss(dev, target_style_image=style, ot_impl="fused_all")
    tr = ConditionedNCATrainer(m, DS(), None, nca_steps=[4, 8], lr=2e-3, pool_size=16, log_base_path="/tmp/ncahip_gpu_test",
                               loss=L, device=dev)
    random.seed(0); np.random.seed(0); torch.manual_seed(0)
    losses = []
    orig = tr.train_batch
    tr.train_batch = lambda b, t: (lambda r: (losses.append(r[1]), r)[1])(orig(b, t))
    tr.train(batch_size=4, epochs=1)
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    ops.check_errors()
