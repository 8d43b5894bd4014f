"""The fused sliced-Wasserstein kernels (csrc/nca_slw.hip, ncahip.loss.sliced_wasserstein_fused) stage by stage against CPU torch and
float64 -- never against the kernels themselves.  The formula is ncahip.loss._sliced_wasserstein's (EncoderConditioning/loss/
appearance_loss.py:121-136) with a stable sort, written out below for a given projection.

Inputs are seeded: relu(randn + 0.3) for feature levels, plain randn for c = 3.  One float64 / fp32-torch record and one set of kernel
outputs is computed per case and shared by the tests of that case.  Every loss carries the upstream factor UP = 0.75 (exact in fp32),
so the backward's g_loss plumbing is part of what is checked.
"""
import functools
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = 0.75

# (c, n, m, B): the smallest shapes at which each mechanism can go wrong
CASES = {
    "image c=3 n=37 m=50": (3, 37, 50, 3),                    # VALU projection, odd lengths, unaligned rows
    "c=64 n=1000 m=1536": (64, 1000, 1536, 2),                # four K chunks, n not a power of two, non-integer resample ratio
    "c=512 n=256 m=256": (512, 256, 256, 2),                  # the widest contraction, one sort call for source and target
    "c=8 n=1 m=1": (8, 1, 1, 1),                              # a row of one element
    "c=4 n=4096 m=4096": (4, 4096, 4096, 2),                  # exactly one LDS chunk
    "c=4 n=20000 m=12345": (4, 20000, 12345, 1),              # past one chunk, padded, global stages, non-integer ratio
    "c=4 n=65536 m=65536": (4, 65536, 65536, 1),              # the largest supported row
    "ties c=64 n=2048 m=2048": (64, 2048, 2048, 2),           # a quarter of the source columns all-zero (half of those -0.0): exact ties
}
NAMES = list(CASES)


def make_inputs(name):
    c, n, m, B = CASES[name]
    g = torch.Generator().manual_seed(1000 + NAMES.index(name))
    if c == 3:
        src, tgt = torch.randn(B, c, n, generator=g), torch.randn(1, c, m, generator=g)
    else:
        src, tgt = torch.relu(torch.randn(B, c, n, generator=g) + 0.3), torch.relu(torch.randn(1, c, m, generator=g) + 0.3)
    if name.startswith("ties"):
        cols = torch.randperm(n, generator=g)[: n // 4]
        src[:, :, cols] = 0.0
        src[:, :, cols[: n // 8]] = -0.0
    proj = F.normalize(torch.randn(c, 32, generator=g), dim=0)
    return src, tgt, proj


def torch_slw(src, tgt, proj):
    """The torch formula for a given projection, stable sort; returns (UP * loss, keys of source, keys of target)"""
    ks, kt = torch.einsum("bcn,cp->bpn", src, proj), torch.einsum("bcn,cp->bpn", tgt, proj)
    ps, pt = ks.sort(dim=-1, stable=True)[0], kt.sort(dim=-1, stable=True)[0]
    return UP * (ps - F.interpolate(pt, src.shape[-1], mode="nearest")).square().sum(), ks, kt


def exact_grad(k64s, k64t, proj64, perm_s, perm_t, jmap):
    """d (UP * loss) / d source in float64 from the closed form, with the given permutations (int64, [B,32,n] and [1,32,m]):
    dk[b, p, perm[b,p,i]] = 2 UP (s - t[j(i)]), dsource = proj . dk, s and t the float64 keys taken through the permutations."""
    s, t = torch.gather(k64s, 2, perm_s), torch.gather(k64t, 2, perm_t)
    res = s - t[:, :, jmap]
    dk = torch.zeros_like(k64s).scatter_(2, perm_s, 2.0 * UP * res)
    return torch.einsum("cp,bpn->bcn", proj64, dk)


def grad_errors(got, ref):
    d = got.double() - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 yardsticks of one case, and the plain fp32 torch path's own errors against them (the bounds derive from those)"""
    from ncahip import ops
    src, tgt, proj = make_inputs(name)
    c, n, m, B = CASES[name]
    s64, t64, p64 = src.double(), tgt.double(), proj.double()
    jmap = ops.slw_nearest_index(m, n).long()
    x = s64.clone().requires_grad_(True)
    loss64, k64s, k64t = torch_slw(x, t64, p64)
    loss64.backward()
    gamma_s = (c + 2) * 2.0 ** -24 * torch.einsum("bcn,cp->bpn", s64.abs(), p64.abs())
    gamma_t = (c + 2) * 2.0 ** -24 * torch.einsum("bcn,cp->bpn", t64.abs(), p64.abs())
    y = src.clone().requires_grad_(True)                      # the plain fp32 torch path on the CPU, same inputs, same projection
    loss32, k32s, k32t = torch_slw(y, tgt, proj)
    loss32.backward()
    perm32_s, perm32_t = k32s.detach().sort(dim=-1, stable=True)[1], k32t.sort(dim=-1, stable=True)[1]
    ex32 = exact_grad(k64s.detach(), k64t, p64, perm32_s, perm32_t, jmap)
    return {"src": src, "tgt": tgt, "proj": proj, "jmap": jmap, "k64s": k64s.detach(), "k64t": k64t, "p64": p64,
            "gamma_s": gamma_s, "gamma_t": gamma_t, "loss64": float(loss64.detach()), "grad64": x.grad,
            "torch_value_err": abs(float(loss32.detach()) - float(loss64.detach())) / float(loss64.detach()),
            "torch_grad_l2": grad_errors(y.grad, x.grad)[0], "torch_exact": grad_errors(y.grad, ex32)}


def run_fused(r):
    from ncahip.autograd import SlicedWasserstein
    from ncahip import ops
    c, n = r["src"].shape[1:]
    m = r["tgt"].shape[2]
    x = r["src"].to(DEV).requires_grad_(True)
    loss = UP * SlicedWasserstein.apply(x, r["tgt"].to(DEV), r["proj"].to(DEV), ops.slw_index_map(m, n, DEV))
    loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


@functools.lru_cache(maxsize=None)
def kernels(name):
    """what the kernels give for one case, stage by stage, downloaded once"""
    from ncahip import ops
    r = reference(name)
    src, tgt, proj = r["src"].to(DEV), r["tgt"].to(DEV), r["proj"].to(DEV)
    ks, kt = ops.slw_project(src, tgt, proj)
    keys_s, keys_t = ks.cpu().clone(), kt.cpu().clone()
    if ks.shape[-1] == kt.shape[-1]:
        _, perm = ops.slw_sort(ks._base)
        perm_s, perm_t = perm[:-1], perm[-1:]
    else:
        perm_s, perm_t = ops.slw_sort(ks)[1], ops.slw_sort(kt)[1]
    jm = ops.slw_index_map(tgt.shape[2], src.shape[2], DEV)
    loss = UP * ops.slw_loss(ks, kt, jm)
    first, second = run_fused(r), run_fused(r)
    torch.cuda.synchronize()
    return {"keys_s": keys_s, "keys_t": keys_t, "sorted_s": ks.cpu(), "sorted_t": kt.cpu(), "perm_s": perm_s.cpu(), "perm_t": perm_t.cpu(),
            "stage_loss": float(loss.cpu()), "loss": float(first[0]), "grad": first[1], "again": second}


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", NAMES)
def test_projection_within_the_dot_product_bound(name):
    """every key within gamma = (c + 2) 2^-24 sum_c |x_c p_c| of the float64 key (the textbook bound of a length-c fp32 dot product in any
    summation order; not a fitted number)"""
    r, k = reference(name), kernels(name)
    for got, ref, gam, what in ((k["keys_s"], r["k64s"], r["gamma_s"], "source"), (k["keys_t"], r["k64t"], r["gamma_t"], "target")):
        assert got.shape == ref.shape
        err = (got.double() - ref).abs()
        worst = float((err / gam.clamp_min(1e-300)).max())
        print(f"projection {name} {what}: worst |error| / gamma {worst:.3f}, worst |error| {float(err.max()):.2e}")
        assert bool((err <= gam).all())


@pytest.mark.parametrize("name", NAMES)
def test_sort_equals_cpu_stable_sort_bit_for_bit(name):
    k = kernels(name)
    for keys, got_v, got_p, what in ((k["keys_s"], k["sorted_s"], k["perm_s"], "source"), (k["keys_t"], k["sorted_t"], k["perm_t"], "target")):
        ref_v, ref_p = torch.sort(keys, dim=-1, stable=True)
        assert got_p.dtype == torch.int32 and got_p.shape == keys.shape
        assert torch.equal(got_p.long(), ref_p), f"{name} {what}: permutation differs from torch.sort(stable=True)"
        assert torch.equal(bits(got_v), bits(ref_v)), f"{name} {what}: sorted values differ in their bits"
    if name.startswith("ties"):
        zeros = int((k["keys_s"] == 0).sum())
        assert zeros >= k["keys_s"].numel() // 4                  # the ties are there: all-zero columns project to exactly 0


@pytest.mark.parametrize("name", NAMES)
def test_loss_value_against_float64(name):
    """bound: ten times the plain fp32 torch path's relative error on the same inputs, or 1e-5, whichever is larger (the convention of
    tests/test_gpu_ot_moment.py).  The value does not depend on the order of equal keys."""
    r, k = reference(name), kernels(name)
    tol = max(10 * r["torch_value_err"], 1e-5)
    e_stage, e_fn = abs(k["stage_loss"] - r["loss64"]) / r["loss64"], abs(k["loss"] - r["loss64"]) / r["loss64"]
    print(f"loss {name}: float64 {r['loss64']:.10e}, kernels rel err {e_fn:.2e} (stages called one by one {e_stage:.2e}), "
          f"fp32 torch rel err {r['torch_value_err']:.2e}, bound {tol:.2e}")
    assert k["stage_loss"] == k["loss"]                          # the autograd function is the same four stages
    assert e_fn <= tol


@pytest.mark.parametrize("name", NAMES)
def test_gradient_against_the_exact_closed_form(name):
    """dsource against the closed form in float64 with the permutation of the CPU's stable sort of the kernels' own fp32 keys, float64
    keys and residuals: no key-order ambiguity is left, so this is the sharp comparison.  Bound as for the value, per measure: ten
    times the plain fp32 torch path's error (against the same closed form with ITS keys' permutation), or 1e-5."""
    r, k = reference(name), kernels(name)
    perm_s = torch.sort(k["keys_s"], dim=-1, stable=True)[1]
    perm_t = torch.sort(k["keys_t"], dim=-1, stable=True)[1]
    ref = exact_grad(r["k64s"], r["k64t"], r["p64"], perm_s, perm_t, r["jmap"])
    l2, mx = grad_errors(k["grad"], ref)
    tol_l2, tol_mx = max(10 * r["torch_exact"][0], 1e-5), max(10 * r["torch_exact"][1], 1e-5)
    print(f"gradient, exact form {name}: rel L2 {l2:.2e} (bound {tol_l2:.2e}), max-abs / max {mx:.2e} (bound {tol_mx:.2e}); "
          f"fp32 torch {r['torch_exact'][0]:.2e}, {r['torch_exact'][1]:.2e}")
    assert bool(torch.isfinite(k["grad"]).all())
    assert l2 <= tol_l2 and mx <= tol_mx


@pytest.mark.parametrize("name", NAMES)
def test_gradient_end_to_end_against_float64_autograd(name):
    """against pure float64 autograd of the torch formula, relative L2 only: two keys that fp32 orders differently from float64 swap two
    gradient entries, a property of the function.  Bound: ten times the plain fp32 torch path's own relative L2 on the same inputs."""
    r, k = reference(name), kernels(name)
    l2, _ = grad_errors(k["grad"], r["grad64"])
    print(f"gradient, end to end {name}: rel L2 {l2:.2e}, fp32 torch {r['torch_grad_l2']:.2e}, bound {10 * r['torch_grad_l2']:.2e}")
    assert l2 <= 10 * r["torch_grad_l2"]


@pytest.mark.parametrize("name", NAMES)
def test_bit_reproducible(name):
    k = kernels(name)
    assert torch.equal(bits(k["again"][0].reshape(1)), bits(torch.tensor([k["loss"]], dtype=torch.float32)))
    assert torch.equal(bits(k["again"][1]), bits(k["grad"]))


def test_loss_module_stream_parity_with_the_torch_path():
    """Loss(appearance_loss_type='SlW') with slw_impl 'fused' and 'torch' from the same torch.manual_seed at 2 x 3 x 64^2: the CPU
    generator ends in the same state, and the appearance terms agree to 1e-5 relative (both paths read the same fp32 VGG features and
    differ only in the sliced-Wasserstein arithmetic, for which 1e-5 is the floor of the value bound above)."""
    from ncahip.loss import Loss
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(64, 64, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        losses = {impl: Loss(dev, target_style_image=style, appearance_loss_type="SlW", slw_impl=impl) for impl in ("torch", "fused")}
    gen0 = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    state0 = torch.rand(2, 16, 64, 64, generator=torch.Generator().manual_seed(2)) * 3 - 1.5
    tgt0 = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    out = {}
    for impl, L in losses.items():
        gen = gen0.to(dev).requires_grad_(True)
        torch.manual_seed(77)
        loss, log = L({"generated_images": gen, "nca_state": state0.to(dev), "target_images": tgt0.to(dev)})
        rng = torch.get_rng_state()
        loss.backward()
        out[impl] = (float(loss), float(log["appearance"]), rng, gen.grad.double().cpu())
    (lt, at, st, gt), (lf, af, sf, gf) = out["torch"], out["fused"]
    rel, l2 = abs(at - af) / abs(at), float((gt - gf).norm() / gt.norm())
    print(f"Loss end to end: loss {lt:.8e} vs {lf:.8e}, appearance {at:.8e} vs {af:.8e} (rel {rel:.2e}), image-gradient rel L2 {l2:.2e}")
    assert torch.equal(st, sf)
    assert rel <= 1e-5 and abs(lt - lf) <= 1e-5 * abs(lt)
    assert bool(torch.isfinite(gf).all())


def test_error_word_is_clean_after_the_module():
    from ncahip import ops
    for name in NAMES:
        kernels(name)
    ops.check_errors()
