"""The WIDE range of the opt-in bf16-MFMA DyNCA forward step (ops.dynca_precision('bf16_wide'): ncahip_dynca_precision mode 1 with
ncahip_dynca_bf16_range 1) against float64 at the smallest shapes of every class it adds:

  per-step   DyncaFwdBf x {<32,128>, <16,256>, <32,256>} x {HAS_COND} x {VEC, any-shape}   (csrc/nca_dynca_bf16_wide.hip)

Reference and caps: test_dynca_bf16_host.py, unchanged (the float64 restatement of the contract, the first-order bound E, cap (a)
|d| <= E (1 + 2^-7) elementwise, cap (b) at most FLIP_FRACTION of the elements beyond FLIP_TOL).  Rows, the instantiation each
reaches, batches (B = ceil(4096 / (H W))), literal seeds and the CPU proof that the float64 restatement and an fp32 evaluation of
the same contract agree within HALF of cap (b) on every (row, pad): test_dynca_bf16_wide_host.py.  Persistent steps are off.

  1  teacher-forced replay, every (row, pad), T = 3: states[t + 1] against contract_step(states[t]) through check_caps; cells whose
     mask is 0 keep their bits, and some cells but not all are idle.
  2  step 0: within E of the float64 oracle step; the same call under 'f32' differs bit-wise; under 'bf16' (narrow) it is the 'f32'
     call bit for bit.
  3  mask sources: in-kernel Philox and packed fire words equal the explicit-uniform run bit for bit.
  4  forms: at W % 4 == 0 an input one float off 16-byte alignment (the any-shape kernel) equals the VEC result bit for bit.
  5  narrow shapes under 'bf16_wide' equal 'bf16' bit for bit: per-step, two-scale, one-launch, steered with an identity field.
  6  edges: (17, 128) and (16, 129) now differ from fp32; (32, 272) under the mode is the fp32 call bit for bit; two-scale and
     steered calls at wide shapes are the fp32 calls.
  7  stylize_clip(precision='bf16_wide') on a C = 20 / fc = 160 edge-conditioned model and on an extra-channel model: the clip
     route, bit-equal to the loop over forward_nsteps inside ops.dynca_precision('bf16_wide').
  8  the worst |d| / E and the worst cap-(b) share per class, printed.

Every test prints its figures (-s)."""
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_dynca_bf16_host import FLIP_FRACTION, bf16_inputs, check_caps, contract_step
from test_dynca_bf16_wide_host import ROW_PADS, ROWS, WIDE, geometry, make_inputs, wide_class, wide_form
from util import REPLAY_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TN = 3
RATE = 0.5
PHILOX_SEED, PHILOX_STEP0 = 0x5EED0004, 9
MODE = "bf16_wide"


def one_pad(row):
    """one pad mode per row for the checks that compare two runs of the kernels with each other: the modes take turns over the rows"""
    return O.PAD_MODES[ROWS.index(row) % len(O.PAD_MODES)]


ROW_ONE_PAD = [(row, one_pad(row)) for row in ROWS]
VEC_ROW_PADS = [(row, pad) for row, pad in ROW_ONE_PAD if WIDE[row][3] == "vec"]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=False) as o:
        yield o
        assert o.set_dynca_precision("f32") == "f32"


@pytest.fixture(autouse=True)
def _after_each(ops):
    yield
    ops.persistent_steps = False
    assert ops.set_dynca_precision("f32") == "f32"           # the test left the mode as it found it
    assert ops.lib().ncahip_dynca_bf16_range(0) == 0
    ops.check_errors()


def _weights(ops, prm, x):
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], x)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def reaches(row):
    """(class, HAS_COND, form) of a row's run"""
    C, fc, cc, _, H, W = geometry(row)
    return wide_class(C, fc), cc > 0, wide_form(H, W)


_RUNS = {}
_WORST = {}      # reaches() -> [worst |d| / E, worst cap-(b) fraction, the (row, pad, step) of each]


def run(ops, row, pad):
    """inputs and the kept history under 'bf16_wide' (T = 3, explicit uniforms) of one (row, pad): computed once, shared, left unchanged"""
    key = (row, pad)
    if key not in _RUNS:
        prm, x, cond, us = make_inputs(row, pad, device=DEV)
        w = _weights(ops, prm, x)
        with ops.dynca_precision(MODE):
            out, states = ops.dynca_nsteps(x, TN, cond, us[:TN], w, pad, RATE, keep_history=True)
        ops.check_errors()
        assert states.shape == (TN + 1,) + tuple(x.shape) and same_bits(states[0], x) and same_bits(states[TN], out)
        _RUNS[key] = dict(prm=prm, x=x, cond=cond, us=us, w=w, states=states.clone())
    return _RUNS[key]


def history(ops, r, pad, us, **kw):
    """the same call as run()'s with other masks or another ambient state; the stored states"""
    return ops.dynca_nsteps(r["x"], TN, r["cond"], us, r["w"], pad, RATE, keep_history=True, **kw)[1]


# ================================================================================================ 1. teacher-forced replay
@pytest.mark.parametrize("row,pad", ROW_PADS)
def test_teacher_forced_replay(ops, row, pad):
    """every stored step against the restatement applied to the kernel's own previous state; idle cells keep their bits"""
    r = run(ops, row, pad)
    states, us = r["states"], r["us"]
    cls = reaches(row)
    assert cls == WIDE[row][1:]
    worst = _WORST.setdefault(cls, [0.0, 0.0, None, None])
    for t in range(TN):
        ref, E = contract_step(states[t], r["cond"], us[t], r["prm"], pad)
        ratio, frac = check_caps(states[t + 1], ref, E, states[t], f"{row} {geometry(row)} {pad} {cls} step {t}")
        if ratio > worst[0]:
            worst[0], worst[2] = ratio, (row, pad, t)
        if frac > worst[1]:
            worst[1], worst[3] = frac, (row, pad, t)
        idle = ((us[t] + RATE).floor() == 0).expand_as(states[t])
        assert torch.equal(states[t + 1].view(torch.int32)[idle], states[t].view(torch.int32)[idle]), (row, pad, t)
        assert bool(idle.any()) and not bool(idle.all())


# ================================================================================================ 2. step 0
@pytest.mark.parametrize("row,pad", ROW_PADS)
def test_step_zero_is_within_E_of_the_exact_step_and_the_mode_ran(ops, row, pad):
    r = run(ops, row, pad)
    x, cond, u, prm = r["x"], r["cond"], r["us"][0], r["prm"]
    p64 = {k: v.double() for k, v in prm.items()}
    exact = O.dynca_step(x.double(), None if cond is None else cond.double(), u, p64, pad, RATE)
    _, E = contract_step(x, cond, u, prm, pad)
    got = r["states"][1]
    d = (got.double() - exact).abs()
    ratio = float((d / E.clamp_min(1e-30))[E > 0].max())
    res = {}
    for mode in ("f32", "bf16"):
        with ops.dynca_precision(mode):
            res[mode] = ops.dynca_nsteps(x, 1, cond, r["us"][:1], r["w"], pad, RATE, keep_history=True)[1][1].clone()
    e32 = rel_err(res["f32"], exact)
    print(f"{row} {pad}: |bf16_wide step - exact step| / E {ratio:.3f} (bound 1), fp32 kernel against the exact step {e32:.2e} "
          f"(bound {REPLAY_TOL:g}), elements the mode changes {int((res['f32'] != got).sum())} of {got.numel()}")
    assert bool((d <= E).all()), ratio
    assert not same_bits(res["f32"], got)
    assert same_bits(res["bf16"], res["f32"])                         # the narrow range leaves a wide shape to the exact kernels
    assert e32 <= REPLAY_TOL


# ================================================================================================ 3. mask sources
@pytest.mark.parametrize("row,pad", ROW_ONE_PAD)
def test_mask_sources_agree(ops, row, pad):
    """explicit uniforms == the same uniforms bit-packed; the in-kernel Philox draw == ops.philox_uniform fed explicitly (and packed)"""
    r = run(ops, row, pad)
    _, _, _, B, H, W = geometry(row)
    pu = torch.stack([ops.philox_uniform(B, H, W, PHILOX_SEED, PHILOX_STEP0 + t) for t in range(TN)])
    assert 0.25 < float((pu + RATE).floor().mean()) < 0.75
    with ops.dynca_precision(MODE):
        packed = history(ops, r, pad, ops.pack_fire_mask(r["us"][:TN], RATE, "dynca"))
        fed = history(ops, r, pad, pu)
        drawn = history(ops, r, pad, None, seed=PHILOX_SEED, step0=PHILOX_STEP0)
        fed_bits = history(ops, r, pad, ops.pack_fire_mask(pu, RATE, "dynca"))
    assert same_bits(packed, r["states"]), (row, pad)
    assert same_bits(drawn, fed) and same_bits(fed_bits, fed), (row, pad)
    assert not same_bits(fed, r["states"])                             # other masks than the table's: the comparison is not vacuous


# ================================================================================================ 4. forms agree
@pytest.mark.parametrize("row,pad", VEC_ROW_PADS)
def test_unaligned_view_equals_the_aligned_call(ops, row, pad):
    """ncahip_dynca_step_fwd_f32 on a contiguous view one float into its buffer: x_in & 15 != 0, so launch_dynca_class picks the
    any-shape kernel although W % 4 == 0.  The two forms differ only in how they stage the state tile into LDS."""
    from ncahip import _capi
    r = run(ops, row, pad)
    C, fc, cc, B, H, W = geometry(row)
    w, cond, u, x = r["w"], r["cond"], r["us"][0].contiguous(), r["x"]
    buf = torch.zeros(x.numel() + 8, device=DEV)
    view = buf[1:1 + x.numel()].view_as(x)
    view.copy_(x)
    assert x.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert wide_form(H, W, x.data_ptr()) == "vec" and wide_form(H, W, view.data_ptr()) == "any"
    L, P, pm = ops.lib(), ops._p, ops.PAD_MODES[pad]
    outs = []
    with ops.dynca_precision(MODE):
        for src in (x, view):
            out = torch.zeros_like(x)
            _capi.check(L.ncahip_dynca_step_fwd_f32(P(src), P(out), P(cond), P(u), P(w.w1), P(w.b1), P(w.w2), P(w.b2), B, C, H, W, fc, cc, pm, RATE,
                                                    0, 0, ops._stream()), "dynca_step_fwd")
            outs.append(out)
    ops.check_errors()
    assert same_bits(outs[0], outs[1]), int((outs[0] != outs[1]).sum())
    assert same_bits(outs[0], r["states"][1])                          # and the first step of the recorded history (held to float64 above)


# ================================================================================================ 5. narrow shapes
NARROW = [("per_step", (12, 96, 3, 2, 11, 35), False, False),
          ("two_scale", (16, 128, 2, 1, 18, 66), True, False),
          ("one_launch", (12, 96, 3, 1, 16, 32), False, True),
          ("one_launch_two_scale", (13, 104, 0, 1, 16, 32), True, True)]


@pytest.mark.parametrize("what,geo,two,persistent", NARROW, ids=[n[0] for n in NARROW])
def test_narrow_shapes_run_what_bf16_runs(ops, what, geo, two, persistent):
    C, fc, cc, B, H, W = geo
    assert ops.dynca_bf16_ok(C, fc)
    prm, x, cond, u = bf16_inputs(C, fc, cc, B, H, W, seed=500 + C, device=DEV)
    us = torch.rand(TN, B, 1, H, W, generator=torch.Generator().manual_seed(501)).to(DEV)
    w = _weights(ops, prm, x)
    res = {}
    for mode in ("f32", "bf16", MODE):
        ops.persistent_steps = persistent
        with ops.dynca_precision(mode):
            out, states = ops.dynca_nsteps(x, TN, cond, us, w, "circular", RATE, two_scale=two)
        assert (states is None) == persistent, "the one-launch kernel did not take the call" if persistent else "unexpected route"
        res[mode] = out.clone()
    ops.persistent_steps = False
    assert same_bits(res[MODE], res["bf16"]), what
    assert not same_bits(res["bf16"], res["f32"])


def test_narrow_steered_shape_runs_what_bf16_runs(ops):
    from ncahip import steer
    C, fc, cc, B, H, W = 12, 96, 3, 2, 11, 35
    prm, x, cond, u = bf16_inputs(C, fc, cc, B, H, W, seed=520, device=DEV)
    w = _weights(ops, prm, x)
    res = {}
    for mode in ("bf16", MODE):
        with ops.dynca_precision(mode):
            res[mode, None] = ops.dynca_nsteps(x, 1, cond, u[None], w, "replicate", RATE, keep_history=True)[1][1].clone()
            for angle in (0.0, 40.0):
                with ops.dynca_direction(steer.direction_field("cartesian", angle, H, W, DEV)):
                    res[mode, angle] = ops.dynca_nsteps(x, 1, cond, u[None], w, "replicate", RATE, keep_history=True)[1][1].clone()
    assert same_bits(res[MODE, 0.0], res["bf16", 0.0]) and same_bits(res[MODE, 40.0], res["bf16", 40.0])
    assert same_bits(res[MODE, 0.0], res[MODE, None])                  # the identity field: the unsteered bits
    assert not same_bits(res[MODE, 40.0], res[MODE, None])


# ================================================================================================ 6. edges
def _one_step(ops, mode, x, cond, u, w, pad="replicate", **kw):
    with ops.dynca_precision(mode):
        return ops.dynca_nsteps(x, 1, cond, u[None], w, pad, RATE, keep_history=True, **kw)[1][1].clone()


@pytest.mark.parametrize("C,fc", [(17, 128), (16, 129)])
def test_just_outside_the_narrow_range_now_differs_from_fp32(ops, C, fc):
    assert not ops.dynca_bf16_ok(C, fc) and ops.dynca_bf16_wide_ok(C, fc)
    prm, x, cond, u = bf16_inputs(C, fc, 2, 1, 6, 8, seed=77 + C, device=DEV)
    w = _weights(ops, prm, x)
    f32, nar, wide = (_one_step(ops, m, x, cond, u, w) for m in ("f32", "bf16", MODE))
    assert same_bits(nar, f32) and not same_bits(wide, f32)
    ref, E = contract_step(x, cond, u, prm, "replicate")
    assert bool(((wide.double() - ref).abs() <= E * (1 + 2.0 ** -7)).all())


def test_outside_both_ranges_is_the_fp32_call(ops):
    C, fc = 32, 272
    assert not ops.dynca_bf16_wide_ok(C, fc)
    prm, x, cond, u = bf16_inputs(C, fc, 3, 1, 6, 8, seed=79, device=DEV)
    w = _weights(ops, prm, x)
    f32, wide = (_one_step(ops, m, x, cond, u, w) for m in ("f32", MODE))
    assert same_bits(wide, f32)
    p64 = {k: v.double() for k, v in prm.items()}
    assert rel_err(f32, O.dynca_step(x.double(), cond.double(), u, p64, "replicate", RATE)) <= REPLAY_TOL


def test_steered_calls_at_wide_shapes_are_the_fp32_calls(ops):
    from ncahip import steer
    C, fc, H, W = 20, 160, 6, 8
    prm, x, cond, u = bf16_inputs(C, fc, 2, 1, H, W, seed=80, device=DEV)
    w = _weights(ops, prm, x)
    with ops.dynca_direction(steer.direction_field("cartesian", 40.0, H, W, DEV)):
        f32, wide = (_one_step(ops, m, x, cond, u, w) for m in ("f32", MODE))
    assert same_bits(wide, f32)
    assert not same_bits(_one_step(ops, MODE, x, cond, u, w), _one_step(ops, "f32", x, cond, u, w))     # unsteered, the mode applies


# ================================================================================================ 7. stylize_clip
def _scale_w2(m):
    with torch.no_grad():
        m.w2.weight.mul_(6.0)
        m.w2.bias.normal_(0.0, 0.02)
    return m


class _FixedCond(torch.nn.Module):
    """stands in for the model's conditioning layer in the hand loop: hands back the map the clip route conditioned the frame on"""

    def __init__(self):
        super().__init__()
        self.cur = None

    def forward(self, img):
        return self.cur


@pytest.mark.parametrize("kind", ["edges", "extra"])
@torch.no_grad()
def test_stylize_clip_bf16_wide_equals_the_loop_over_forward_nsteps(ops, kind):
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    from ncahip.models.dynca_extra import DyNCA as ExtraDyNCA
    Fn, H, W, step_n = 3, 32, 32, 3
    torch.manual_seed(3)
    if kind == "extra":
        m = _scale_w2(ExtraDyNCA(21, 3, fc_dim=160, padding_mode="circular", pos_emb="CPE", perception_scales=[0], device=torch.device(DEV)))
    else:
        m = _scale_w2(DyNCA(20, 3, fc_dim=160, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
                            device=torch.device(DEV)))
    assert not ops.dynca_bf16_ok(m.c_in, 160) and ops.dynca_bf16_wide_ok(m.c_in, 160)
    m.mask_rng, m.mask_seed = "philox", 11
    frames = (torch.rand(Fn, 3, H, W, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    res = {}
    for precision in (MODE, "f32"):
        m._mask_step = 40
        imgs, h = video.stylize_clip(m, frames, step_n=step_n, precision=precision)
        assert video.stylize_clip.last_path == "clip" and m._mask_step == 40 + Fn * step_n
        assert ops.set_dynca_precision("f32") == "f32"                       # the process mode is what it was before
        res[precision] = (imgs.clone(), h.clone())
    assert not torch.equal(res[MODE][1], res["f32"][1])
    # the loop over forward_nsteps under the context manager: the same Philox masks, the conditioning maps of the clip route
    m._mask_step = 40
    h = m.seed(1, size=(W, H))
    want = []
    layer = m.cond_layer
    try:
        with ops.dynca_precision(MODE):
            if kind == "extra":
                gray = ops.clip_gray(frames.unsqueeze(1), "mean")
            else:
                bank = torch.cat((layer.sobel_x.weight, layer.sobel_y.weight, layer.laplacian.weight), dim=0)
                cond = ops.clip_cond(frames.unsqueeze(1), bank, "mean", True)
                m.cond_layer = _FixedCond()
            for n in range(Fn):
                if kind == "extra":
                    x, rgb = m.forward_nsteps(torch.cat((h, gray[n][:, None]), 1), step_n)
                    h = x[:, :-1].contiguous()
                else:
                    m.cond_layer.cur = cond[n]
                    h, rgb = m.forward_nsteps(h, step_n, cond_img=frames[n:n + 1].mean(1, keepdim=True))
                    h = h.clone()
                want.append((rgb.float().clamp(-1.0, 1.0) + 1.0) / 2.0)
    finally:
        m.cond_layer = layer
    want = torch.cat(want)
    assert m._mask_step == 40 + Fn * step_n
    assert res[MODE][0].shape == want.shape and torch.equal(res[MODE][0], want) and torch.equal(res[MODE][1], h)
    assert float(want.std()) > 1e-3


# ================================================================================================ 8. the figures per class
def test_print_the_worst_figures_per_class(ops):
    """what the replays above measured, per instantiation (DESIGN.md quotes this table); asserts nothing the replays did not"""
    print()
    for cls in sorted(_WORST, key=str):
        (cp, fcp), has_cond, form = cls
        ratio, frac, at_ratio, at_frac = _WORST[cls]
        print(f"[bf16 wide] DyncaFwdBf <{cp},{fcp},{str(has_cond).lower()}> {form}: worst |d| / E {ratio:.3f} at {at_ratio}, "
              f"worst cap-(b) fraction {100 * frac:.3f} % at {at_frac} (cap {100 * FLIP_FRACTION:g} %)")
        assert ratio <= 1 + 2.0 ** -7 and frac <= FLIP_FRACTION
