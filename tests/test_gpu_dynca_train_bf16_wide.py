"""The WIDE range of the bf16-MFMA TRAINING mode of DyNCA on the device (include/ncahip.h, "bf16-MFMA training, the WIDE range"): the
stage entry points ncahip_dynca_step_bwd_bfmma_wide_f32 and ncahip_gram_rows_bf16_wide held to the stage caps of
test_dynca_train_bf16_host.py (every stage fed the kernel's own previous stage), the gate against the wide FORWARD's, the driver against
a Python loop over the stage entries, against itself, against the float64 contract and against the exact backward on the same history,
and the route through autograd, the models and DyNCATrainer.  Case rows, seeds and the close-to-fp32 literal are
test_dynca_train_bf16_wide_host.py's; every test prints its figures (-s)."""
import pytest
import torch

from gpu_ops import gpu_ops
from test_dynca_train_bf16_host import RATE, _rb, check_gram, check_t1, from_bits, rel_l2, run_stage_checks
from test_dynca_train_bf16_wide_host import CLOSE_TO_F32_WIDE, NARROW_ROW, ROWS, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("x0", "w1", "b1", "w2", "b2")
PHILOX_SEED, PHILOX_STEP = 0x5EED0042, 5


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=False) as o:
        yield o
        assert o.set_dynca_precision("f32") == "f32"


@pytest.fixture(autouse=True)
def _after_each(ops):
    yield
    assert ops.set_dynca_precision("f32") == "f32"           # the test left the ambient mode as it found it
    ops.check_errors()


def _weights(ops, prm, x):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x)


def step_entry(ops, c, x, g, u, seed=0, step=0, gw2=None, narrow=False):
    """ncahip_dynca_step_bwd_bfmma_wide_f32 (narrow: the narrow entry): dict y, dh (int16 bit patterns), dy, gx, gw2.  u: fp32 uniforms,
    int32 packed bits (with seed = SEED_U_IS_BITS) or None (Philox).  gw2 given: accumulated into."""
    from ncahip import _capi
    B, C, fc, cc, H, W = c["dims"]
    w = _weights(ops, c["prm"], x)
    L, P = ops.lib(), ops._p
    sfx = "" if narrow else "_wide"
    y = torch.full((B, 4 * C, H, W), 0x7fc0, device=DEV, dtype=torch.int16)        # NaN patterns: every element must be written
    dh = torch.full((B, fc, H, W), 0x7fc0, device=DEV, dtype=torch.int16)
    dy = torch.full((B, 4 * C, H, W), float("nan"), device=DEV)
    gx = torch.full_like(g, float("nan"))
    acc = gw2 is not None
    gw2 = torch.full((C * fc + C,), float("nan"), device=DEV) if gw2 is None else gw2
    nws = getattr(L, f"ncahip_dynca_step_bwd_bfmma{sfx}_workspace")(B, C, H, W, fc)
    assert nws > 0
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    _capi.check(getattr(L, f"ncahip_dynca_step_bwd_bfmma{sfx}_f32")(P(x), P(c["cond"]), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc,
                                                                    ops.PAD_MODES[c["pad"]], RATE, seed, step, P(g), P(gx), P(y), P(dh), P(dy),
                                                                    P(gw2), int(acc), P(ws), nws, ops._stream()), "step_bwd_bfmma" + sfx)
    return dict(y=y, dh=dh, dy=dy, gx=gx, gw2=gw2)


def gram_entry(ops, c, dh, y, out=None, narrow=False):
    """ncahip_gram_rows_bf16_wide(dh, y, cond): [dW1 | db1]; out given: accumulated into"""
    from ncahip import _capi
    B, C, fc, cc, H, W = c["dims"]
    L, P = ops.lib(), ops._p
    sfx = "" if narrow else "_wide"
    nb = 4 * C + cc
    acc = out is not None
    out = torch.full((fc * nb + fc,), float("nan"), device=DEV) if out is None else out
    nws = getattr(L, f"ncahip_gram_rows_bf16{sfx}_workspace")(fc, nb, B, H * W)
    ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
    _capi.check(getattr(L, f"ncahip_gram_rows_bf16{sfx}")(P(dh), fc, P(y), 4 * C, P(c["cond"]), cc, B, H * W, P(out), int(acc), P(ws), nws,
                                                          ops._stream()), "gram_bf16" + sfx)
    return out


def stages(ops, c, u, **kw):
    r = step_entry(ops, c, c["x"], c["g_final"], u, **kw)
    r["gram"] = gram_entry(ops, c, r["dh"], r["y"])
    ops.check_errors()
    return r


def as_values(r):
    return dict(r, y=from_bits(r["y"]), dh=from_bits(r["dh"]))


# ================================================================================================ stage by stage
@pytest.mark.parametrize("row", list(ROWS))
def test_stages_inside_their_caps(ops, row):
    c = make_case(row, device=DEV)
    r = stages(ops, c, c["us"][0].contiguous())
    run_stage_checks(as_values(r), c)


def test_stages_with_every_fire_mask_source(ops):
    """row c32fc96: explicit u (above), packed bits (the same bits as explicit u) and Philox (u = None) through all stage caps"""
    from ncahip import _capi
    c = make_case("c32fc96", device=DEV)
    B, C, fc, cc, H, W = c["dims"]
    ref = stages(ops, c, c["us"][0].contiguous())
    bits = ops.pack_fire_mask(c["us"][:1].contiguous(), RATE, "dynca")
    r = stages(ops, c, bits, seed=_capi.SEED_U_IS_BITS)
    for k in ("y", "dh", "dy", "gx", "gw2", "gram"):
        assert torch.equal(r[k], ref[k]), k
    run_stage_checks(as_values(r), c)
    r = stages(ops, c, None, seed=PHILOX_SEED, step=PHILOX_STEP)
    cp = dict(c, us=ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP, DEV)[None])
    assert not torch.equal(r["dh"], ref["dh"])            # another mask
    run_stage_checks(as_values(r), cp)


def test_narrow_shapes_run_the_narrow_kernels(ops):
    """inside the narrow range both wide stage entries are torch.equal to the narrow ones"""
    c = make_case("narrow", device=DEV, dims=NARROW_ROW, seed=11)
    u = c["us"][0].contiguous()
    a = step_entry(ops, c, c["x"], c["g_final"], u)
    b = step_entry(ops, c, c["x"], c["g_final"], u, narrow=True)
    a["gram"], b["gram"] = gram_entry(ops, c, a["dh"], a["y"]), gram_entry(ops, c, b["dh"], b["y"], narrow=True)
    for k in ("y", "dh", "dy", "gx", "gw2", "gram"):
        assert torch.equal(a[k], b[k]), k


def test_gram_bf16_wide_alone(ops):
    """ncahip_gram_rows_bf16_wide on operands of its own at shapes the step never gives it: HW % 8 != 0 (element loads), ma = 129 and 256,
    nb = 80 and 132, nb2 = 0, more chunks than workgroups can take in one trip; its accumulate flag; and the old entry inside its range"""
    from ncahip import _capi
    L, P = ops.lib(), ops._p
    g = torch.Generator().manual_seed(3)

    def run(fn, wsfn, a, b1, b2, out, acc):
        B, ma, H, W = a.shape
        nb1, nb2 = b1.shape[1], 0 if b2 is None else b2.shape[1]
        nws = getattr(L, wsfn)(ma, nb1 + nb2, B, H * W)
        assert nws > 0
        ws = torch.empty(nws, device=DEV, dtype=torch.uint8)
        _capi.check(getattr(L, fn)(P(a), ma, P(b1), nb1, P(b2), nb2, B, H * W, P(out), acc, P(ws), nws, ops._stream()), fn)

    for B, ma, nb1, nb2, H, W in [(2, 129, 80, 0, 6, 10), (1, 256, 128, 4, 7, 9), (3, 160, 80, 2, 256, 160), (1, 256, 129, 3, 4, 8),
                                  (1, 130, 15, 0, 4, 8), (1, 96, 48, 3, 16, 16)]:
        a = torch.randn(B, ma, H, W, generator=g).to(torch.bfloat16).to(DEV)
        b1 = torch.randn(B, nb1, H, W, generator=g).to(torch.bfloat16).to(DEV)
        b2 = torch.randn(B, nb2, H, W, generator=g).to(DEV) if nb2 else None
        nb = nb1 + nb2
        out = torch.full((ma * nb + ma,), float("nan"), device=DEV)
        run("ncahip_gram_rows_bf16_wide", "ncahip_gram_rows_bf16_wide_workspace", a, b1, b2, out, 0)
        b = b1.double() if b2 is None else torch.cat([b1.double(), _rb(b2.double())], dim=1)
        check_gram(out, a, b, f"gram_rows_bf16_wide B={B} ma={ma} nb={nb1}+{nb2} HW={H * W}")
        first = out.clone()
        run("ncahip_gram_rows_bf16_wide", "ncahip_gram_rows_bf16_wide_workspace", a, b1, b2, out, 1)
        assert torch.equal(out, first + first)
        if ma == 96 and nb == 51:                   # inside the old range: the old launcher
            old = torch.full_like(first, float("nan"))
            run("ncahip_gram_rows_bf16", "ncahip_gram_rows_bf16_workspace", a, b1, b2, old, 0)
            assert torch.equal(old, first)


# ================================================================================================ gate consistency
@pytest.mark.parametrize("row", ["c32fc96", "fc144", "c32fc256"])
def test_gate_is_the_forwards(ops, row):
    """dh_out is zero exactly where relu of the WIDE FORWARD's layer-1 pre-activation is zero.  The forward's hb is read through a probe:
    a forward step under dynca_precision("bf16_wide") on the same input whose w2 selects C hidden units at a time with weight 2^30 (exact
    in bf16; b2 = 0), so that x' - x is nonzero wherever hb is, on the firing cells.  Rows c32fc96 (forward class <32, 128>, K1Q = 5),
    fc144 (<16, 256>: the slices must be <16, 128>) and c32fc256 (<32, 256>): this holds the slice design to the forward's class."""
    c = make_case(row, device=DEV)
    B, C, fc, cc, H, W = c["dims"]
    u = c["us"][0].contiguous()
    r = as_values(step_entry(ops, c, c["x"], c["g_final"], u))
    fire = (u + RATE).floor().bool().expand(B, fc, H, W)
    hb_nz = torch.zeros(B, fc, H, W, device=DEV, dtype=torch.bool)
    with ops.dynca_precision("bf16_wide"):
        for j0 in range(0, fc, C):
            n = min(C, fc - j0)
            w2 = torch.zeros(C, fc, 1, 1, device=DEV)
            w2[torch.arange(n), j0 + torch.arange(n)] = 2.0 ** 30
            w = ops.DyncaWeights(c["prm"]["w1.weight"], c["prm"]["w1.bias"], w2, torch.zeros(C, device=DEV), c["x"])
            out = ops.dynca_step(c["x"], c["cond"], u, w, c["pad"], RATE)
            hb_nz[:, j0:j0 + n] = ((out - c["x"]) != 0)[:, :n]
    w2b = _rb(c["prm"]["w2.weight"].double()[:, :, 0, 0])
    gb = _rb(c["g_final"].double() * fire[:, :1])
    back = torch.einsum("cj,bchw->bjhw", w2b, gb).abs() > 2.0 ** -100          # W2b^T gb itself is not zero
    dh_nz = r["dh"] != 0
    print(f"gate: {int(fire.sum())} firing units, {int((hb_nz & fire).sum())} open; dh_out nonzero on {int(dh_nz.sum())}")
    assert not bool((dh_nz & ~fire).any())                       # nothing flows where the cell did not fire
    assert not bool((dh_nz & fire & ~hb_nz).any())               # closed in the forward -> zero
    assert not bool((hb_nz & fire & back & ~dh_nz).any())        # open in the forward -> not zero
    assert 0.2 < float((hb_nz & fire).sum() / fire.sum()) < 0.8


# ================================================================================================ the driver
_HIST = {}


def history(ops, row):
    """inputs and the wide mode-1 history (T = 3, explicit uniforms) of a row: computed once, shared, left unchanged"""
    if row not in _HIST:
        c = make_case(row, device=DEV) if row in ROWS else make_case(row, device=DEV, dims=NARROW_ROW, seed=11)
        w = _weights(ops, c["prm"], c["x"])
        with ops.dynca_precision("bf16_wide"):
            _, states = ops.dynca_nsteps(c["x"], 3, c["cond"], c["us"], w, c["pad"], RATE, keep_history=True)
        with ops.dynca_precision("f32"):
            _, exact = ops.dynca_nsteps(c["x"], 3, c["cond"], c["us"], w, c["pad"], RATE, keep_history=True)
        assert not torch.equal(states[1], exact[1])               # the mode ran
        _HIST[row] = dict(c=c, w=w, states=states.clone())
    return _HIST[row]


def driver(ops, h, T, g_states=None, precision="bf16_wide"):
    c = h["c"]
    states = h["states"][:T + 1].contiguous()
    gs = None if g_states is None else g_states[:T + 1].contiguous()
    return ops.dynca_nsteps_backward(states, c["cond"], c["us"][:T].contiguous(), h["w"], c["g_final"], gs, T, c["pad"], RATE,
                                     precision=precision)


def quiet_g_states(c, T):
    """cotangents of the intermediate states that are zero on the cells that fire at their step (see the narrow file): the driver forms
    (g + g_states[t]) + adjoint inside its stencil kernel, the loop can only hand g + g_states[t] to the step entry"""
    gs = c["g_states"].clone()
    for t in range(T):
        gs[t] = gs[t] * (1 - (c["us"][t] + RATE).floor())
    gs[T] = 0
    return gs


@pytest.mark.parametrize("row,T", [("c17", 1), ("c17", 3), ("fc144", 1), ("fc144", 3), ("c32fc256", 1), ("c32fc256", 3)])
def test_driver_equals_the_loop_over_the_stage_entries(ops, row, T):
    """ncahip_dynca_nsteps_bwd_bfmma_wide_f32 (T = 3: with quiet g_states) is torch.equal to the Python loop over the single-step entry,
    the gram entry and the existing adjoint in the driver's accumulate order; two runs are torch.equal"""
    h = history(ops, row)
    c = h["c"]
    B, C, fc, cc, H, W = c["dims"]
    gs = quiet_g_states(c, T) if T > 1 else None
    got = driver(ops, h, T, gs)
    again = driver(ops, h, T, gs)
    ops.check_errors()
    gw2 = torch.zeros(C * fc + C, device=DEV)
    gw1 = torch.zeros(fc * (4 * C + cc) + fc, device=DEV)
    g = c["g_final"]
    for t in range(T - 1, -1, -1):
        gin = g if gs is None else g + gs[t]
        r = step_entry(ops, c, h["states"][t].contiguous(), gin, c["us"][t].contiguous(), gw2=gw2)
        gram_entry(ops, c, r["dh"], r["y"], out=gw1)
        g = r["gx"]
    loop = dict(x0=g, w1=gw1[:fc * (4 * C + cc)].view(fc, -1), b1=gw1[fc * (4 * C + cc):], w2=gw2[:C * fc].view(C, fc), b2=gw2[C * fc:])
    for k in KEYS:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], again[k]), f"{k}: two runs differ"
        assert torch.equal(got[k], loop[k]), f"{k}: driver differs from the loop, max {float((got[k] - loop[k]).abs().max()):.3e}"


@pytest.mark.parametrize("row", ["c20", "fc256"])
def test_t3_driver_equals_a_chain_of_t1_drivers(ops, row):
    """T = 3 with the FULL g_states (firing cells included) is torch.equal to three T = 1 driver calls chained through dL/dx, their
    weight gradients added in the driver's order ((s2 + s1) + s0)"""
    h = history(ops, row)
    c = h["c"]
    gs = c["g_states"]
    got = driver(ops, h, 3, gs)
    g, acc = c["g_final"], None
    for t in (2, 1, 0):
        st = torch.stack([h["states"][t], h["states"][t + 1]])
        r = ops.dynca_nsteps_backward(st, c["cond"], c["us"][t:t + 1].contiguous(), h["w"], g, torch.stack([gs[t], torch.zeros_like(gs[t])]), 1,
                                      c["pad"], RATE, precision="bf16_wide")
        g = r["x0"]
        acc = {k: r[k].clone() if acc is None else acc[k] + r[k] for k in KEYS[1:]}
    chain = dict(x0=g, **acc)
    for k in KEYS:
        assert torch.equal(got[k], chain[k]), f"{k}: max {float((got[k] - chain[k]).abs().max()):.3e}"


@pytest.mark.parametrize("row", ["c20", "c32fc256"])
def test_t1_driver_against_the_float64_contract(ops, row):
    """one backward step through the driver (g_states slot 0 included) against contract_backward in float64, every gradient tensor under
    the tolerance test_dynca_train_bf16_host.t1_reference derives for the case"""
    c = make_case(row, 1, device=DEV)
    w = _weights(ops, c["prm"], c["x"])
    with ops.dynca_precision("bf16_wide"):
        _, states = ops.dynca_nsteps(c["x"], 1, c["cond"], c["us"], w, c["pad"], RATE, keep_history=True)
    got = ops.dynca_nsteps_backward(states, c["cond"], c["us"], w, c["g_final"], c["g_states"], 1, c["pad"], RATE, precision="bf16_wide")
    check_t1({k: v.cpu() for k, v in got.items()}, make_case(row, 1), row)


@pytest.mark.parametrize("row", list(ROWS))
def test_close_to_the_exact_backward_on_the_same_history(ops, row):
    """each gradient tensor against ncahip_dynca_nsteps_bwd_f32 on the SAME (wide mode-1) history: relative L2 under the host file's
    literal (twice the worst distance of the float64 contract from the float64 exact gradients)"""
    h = history(ops, row)
    gs = h["c"]["g_states"]
    got, ref = driver(ops, h, 3, gs), driver(ops, h, 3, gs, precision="f32")
    e = {k: rel_l2(got[k], ref[k]) for k in KEYS}
    print(f"{row}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + f"  (cap {CLOSE_TO_F32_WIDE:g})")
    assert max(e.values()) <= CLOSE_TO_F32_WIDE, e
    assert max(e.values()) > 1e-5                # the two backwards are different kernels


def test_on_a_narrow_row_the_wide_driver_is_the_narrow_driver(ops):
    h = history(ops, "narrow")
    gs = h["c"]["g_states"]
    wide, narrow = driver(ops, h, 3, gs), driver(ops, h, 3, gs, precision="bf16")
    for k in KEYS:
        assert torch.equal(wide[k], narrow[k]), k


# ================================================================================================ through autograd
def _model(C=20, fc=160, pad="circular", scaled=True):
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(5)
    m = DyNCA(C, 3, fc_dim=fc, padding_mode=pad, conditioning="pos_emb", device=torch.device(DEV))
    if scaled:
        with torch.no_grad():                  # the shipped initialisation has w2 ~ 0.1 gain and zero bias: make every gradient carry weight
            m.w1.weight.mul_(4.0)
            m.w2.weight.mul_(8.0)
    m.mask_rng, m.mask_seed = "philox", 77
    return m


def _grads(m, x, T):
    m._mask_step = 0
    for p in m.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    out, _ = m.forward_nsteps(xin, T)
    (out * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum().backward()
    return out.detach(), dict(x0=xin.grad, w1=m.w1.weight.grad[:, :, 0, 0], b1=m.w1.bias.grad, w2=m.w2.weight.grad[:, :, 0, 0], b2=m.w2.bias.grad)


def _direct(ops, m, x, T, precs):
    cond = m._cond(x, None)
    w = ops.DyncaWeights(m.w1.weight.detach(), m.w1.bias.detach(), m.w2.weight.detach(), m.w2.bias.detach(), x)
    cot = torch.linspace(-1, 1, x.numel(), device=DEV).view_as(x)
    direct = {}
    for prec in precs:
        with ops.dynca_precision(prec):
            out, states = ops.dynca_nsteps(x, T, cond, None, w, m.padding_mode, 0.5, m.mask_seed, 0, keep_history=True)
        direct[prec] = (out.clone(), ops.dynca_nsteps_backward(states, cond, None, w, cot, None, T, m.padding_mode, 0.5, m.mask_seed, 0,
                                                               precision=prec), states.clone())
    return cond, direct


def test_autograd_route(ops):
    """train_precision = "bf16_wide" at C = 20 / fc = 160: output, history and gradients are the direct ops call's; "f32": the exact route's"""
    from ncahip.autograd import dynca_nsteps_autograd
    T = 3
    m = _model()
    x = (torch.rand(2, 20, 16, 32, generator=torch.Generator().manual_seed(9)) - 0.5).to(DEV)
    cond, direct = _direct(ops, m, x, T, ("f32", "bf16_wide"))
    assert not torch.equal(direct["f32"][0], direct["bf16_wide"][0])
    for prec in ("bf16_wide", "f32"):
        m.train_precision = prec
        with ops.dynca_precision("bf16_wide" if prec == "f32" else "f32"):          # the ambient mode is ignored by autograd
            out, g = _grads(m, x, T)
        assert torch.equal(out, direct[prec][0]), prec
        for k in KEYS:
            assert torch.equal(g[k], direct[prec][1][k]), (prec, k)
        m._mask_step = 0
        _, kept = dynca_nsteps_autograd(m, x.clone().requires_grad_(True), cond, T, 0.5, want_states=True)
        assert kept.shape[0] == T + 1 and torch.equal(kept.detach(), direct[prec][2]), prec
    m.train_precision = "bf16"                    # the narrow value at a wide shape: the exact route, bit for bit
    out, g = _grads(m, x, T)
    assert torch.equal(out, direct["f32"][0])
    for k in KEYS:
        assert torch.equal(g[k], direct["f32"][1][k]), k


@pytest.mark.parametrize("C,fc,same_as", [(12, 96, "bf16"), (33, 96, "f32")])
def test_inside_the_narrow_range_and_outside_the_wide_one(ops, C, fc, same_as):
    """C = 12 / fc = 96: "bf16_wide" is "bf16" bit for bit.  C = 33: "bf16_wide" is "f32" -- the fused kernels stop at C = 32, so what
    both settings do there is the exact route's refusal, the same error word for word (the setting adds no route and no error)"""
    from ncahip import _capi
    from ncahip.autograd import dynca_train_precision
    m = _model(C, fc)
    x = (torch.rand(1, C, 16, 16, generator=torch.Generator().manual_seed(C)) - 0.5).to(DEV)

    def run(prec):
        m.train_precision = prec
        try:
            return _grads(m, x, 2)
        except _capi.NcaHipError as e:
            return str(e)
    m.train_precision = "bf16_wide"
    assert dynca_train_precision(m, x) == same_as
    r0, r1 = run(same_as), run("bf16_wide")
    if C > 32:
        assert isinstance(r0, str) and r0 == r1 and "C=33" in r0, (r0, r1)
        return
    (out0, g0), (out1, g1) = r0, r1
    assert torch.equal(out0, out1)
    for k in KEYS:
        assert torch.equal(g0[k], g1[k]), k


def test_an_attached_direction_field_is_refused(ops):
    from ncahip import _capi
    h = history(ops, "c20")
    B, C, fc, cc, H, W = h["c"]["dims"]
    dirs = torch.zeros(1, 2, H, W, device=DEV)
    dirs[:, 1] = 1
    with ops.dynca_direction(dirs):
        with pytest.raises(_capi.NcaHipError, match="direction field"):
            driver(ops, h, 1)
    driver(ops, h, 1)                     # detached again: runs


def test_a_bf16_pool_with_bf16_wide_training_raises(ops):
    m = _model()
    m.train_precision = "bf16_wide"
    x = torch.zeros(1, 20, 16, 16, device=DEV, dtype=torch.bfloat16).requires_grad_(True)
    with pytest.raises(ValueError, match="bf16_wide"):
        m.forward_nsteps(x, 2)


def test_trainer_steps_in_bf16_wide(ops):
    """three DyNCATrainer.step iterations with train_precision="bf16_wide" on a C = 20 / fc = 160 model: finite loss, changed parameters,
    a written-back pool"""
    from ncahip.dynca_trainer import DyNCATrainer
    m = _model(scaled=False)                   # the shipped initialisation, as a training run starts
    m.seed_mode = "random"
    target = torch.linspace(-0.5, 0.5, 20, device=DEV).view(1, 20, 1, 1)
    tr = DyNCATrainer(m, lambda d: ((d["nca_state"] - target) ** 2).mean(), pool_size=8, size=(32, 16), batch_size=2, nca_steps=(2, 5),
                      device=torch.device(DEV), train_precision="bf16_wide")
    assert m.train_precision == "bf16_wide"
    before = [p.detach().clone() for p in m.parameters()]
    pool0 = tr.pool.clone()
    losses = [float(tr.step()[0]) for _ in range(3)]
    print("losses", losses)
    assert all(l == l and abs(l) < float("inf") for l in losses)
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, m.parameters()))
    assert not torch.equal(pool0, tr.pool) and bool(torch.isfinite(tr.pool).all())
