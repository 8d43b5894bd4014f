"""GPU tests of clip stylisation with ConditionedNCA models on a bf16 state (ncahip_clip_encode_bf16, ncahip_clip_emit_unit_bf16,
ncahip_cond_finalize_emit_bf16, ncahip_cond_clip_bf16, stylize_clip_conditioned(precision='bf16')): each new launch bit for bit against
the launches it replaces, the driver's bookkeeping bit for bit against a Python loop over the existing bf16 entry points, continuation
and chunking, the whole function against the hand loop, the sticky error word, and one frame against float64."""
import copy

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from util import near_threshold

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
FORMATS = [(torch.float32, "rgb24"), (torch.uint8, "rgb24"), (torch.uint8, "i420"), (torch.uint8, "nv12")]


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:
        yield o


def _same(a, b):
    """bit for bit, NaN and the sign of a zero included"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {torch.float32: torch.int32, BF: torch.int16}.get(a.dtype)
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view)) if view else torch.equal(a, b)


def _encoder(E, ch, seed, bias=None):
    from ncahip.encoder import ImageEncoder
    torch.manual_seed(seed)
    enc = ImageEncoder(E, ch)
    if bias is not None:
        with torch.no_grad():
            enc.embed[0].bias.fill_(bias)
    return enc


# ------------------------------------------------------------------ 1. encoder: the fp32 kernel's goal, rounded on the store
@pytest.mark.parametrize("E", [8, 16, 28])
def test_clip_encode_bf16_is_the_rounded_fp32_goal(ops, E):
    enc = _encoder(E, 3, E)
    for Fn, B, H, W in ((1, 1, 1, 1), (2, 1, 5, 7), (1, 2, 16, 16), (1, 1, 17, 33)):
        gen = torch.Generator().manual_seed(H * 100 + W)
        for frames in (torch.rand(Fn, B, 3, H, W, generator=gen).to(DEV), torch.randint(0, 256, (Fn, B, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)):
            got = ops.clip_encode(frames, enc, dtype=BF)
            assert got.dtype == BF and got.shape == (Fn, B, E, H, W)
            assert _same(got, ops.clip_encode(frames, enc).to(BF)), (E, Fn, B, H, W, frames.dtype)
    # the padding trap of the fp32 test: with a bias of +0.5 relu(b1 + ...) is far from 0 on the halo, conv2 must still see zeros there
    encb = _encoder(E, 3, E + 1, bias=0.5)
    frames = torch.rand(2, 1, 3, 5, 7, generator=torch.Generator().manual_seed(7)).to(DEV)
    assert _same(ops.clip_encode(frames, encb, dtype=BF), ops.clip_encode(frames, encb).to(BF))
    with pytest.raises(TypeError):
        ops.clip_encode(frames, enc, dtype=torch.float16)
    ops.check_errors()


# ------------------------------------------------------------------ 2. image of a bf16 state
def _bf16_specials(with_nan):
    """the special values of test_clip_emit_unit_is_exact that bf16 holds: both zeros, 1, values beyond both ends, the infinities, (NaN,)
    and for several k the bf16 value nearest k / 255 with its two bf16 neighbours"""
    ks = (torch.tensor([1, 2, 3, 64, 127, 128, 200, 254, 255], dtype=torch.float32) / 255.0).to(BF)
    bits = ks.view(torch.int16)
    near = torch.cat([bits - 1, bits, bits + 1]).view(BF)
    one = torch.tensor([1.0], dtype=BF).view(torch.int16)
    special = torch.tensor([-0.0, 0.0, 1.0, -1e-30, 1e-30, -3.0, 3.0, 0.5, float("-inf"), float("inf")] + ([float("nan")] if with_nan else []), dtype=BF)
    return torch.cat([special, torch.cat([one - 1, one + 1]).view(BF), near])


@pytest.mark.parametrize("B,C,H,W", [(2, 5, 6, 12), (1, 20, 16, 16)])
def test_clip_emit_unit_of_a_bf16_state_is_the_fp32_emit_of_the_widened_state(ops, B, C, H, W):
    gen = torch.Generator().manual_seed(C + W)
    for out_dtype, out_format in FORMATS:
        x = (torch.rand(B, C, H, W, generator=gen) * 1.6 - 0.3).to(BF)          # beyond [0, 1] on both sides
        v = _bf16_specials(out_dtype == torch.float32)
        n = min(v.numel(), H * W)
        for c in range(3):
            x[:, c].reshape(B, -1)[:, :n] = v.roll(7 * c)[:n]
        x = x.to(DEV)
        got = ops.clip_emit_unit(x, out_dtype, out_format)
        want = ops.clip_emit_unit(x.float(), out_dtype, out_format)
        assert _same(got, want), (out_dtype, out_format)
        if out_dtype == torch.float32:
            assert bool(torch.isnan(got).any()) and float(got[~torch.isnan(got)].max()) == 1.0
    ops.check_errors()


# ------------------------------------------------------------------ 3. finalize + image in one launch
def _weights(ops, C, seed, like):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    return ops.CondWeights(r(3 * C, 1, 3, 3, k=0.3), r(64, 3 * C, 1, 1, k=0.14), r(64, k=0.1), r(64, 64, 1, 1, k=0.12), r(64, k=0.1),
                           r(C, 64, 1, 1, k=0.04), like)


def _dense_state(B, C, H, W, gen):
    x = torch.rand(B, C, H, W, generator=gen) * 0.8
    x[:, 3] = 1.0                   # alive everywhere: every cell does real work
    return x.to(DEV)


def _built_pending(B, C, H, W, gen):
    """A pending state made to hit the finalize's edges: alpha just above (bf16(0.1) = 0.10009...) and just below (0.0996...) the
    threshold in the corners and along the edges (a neighbour outside the image does not count), dead stretches in between, pre = 0
    cells next to alive ones, values beyond +-10."""
    x = torch.randn(B, C, H, W, generator=gen) * 6.0
    a = torch.zeros(B, H, W)
    above, below = 0.10009765625, 0.099609375
    a[:, 0, 0], a[:, 0, W - 1], a[:, H - 1, 0], a[:, H - 1, W - 1] = above, below, below, above
    a[:, 0, W // 2], a[:, H - 1, W // 2 - 1], a[:, H // 2, 0], a[:, H // 2 - 1, W - 1] = above, below, above, 0.5
    a[:, H // 2, W // 2] = 0.5
    x[:, 3] = a
    pre = torch.ones(B, H, W, dtype=torch.uint8)
    pre[:, 0, 1], pre[:, H // 2, W // 2 + 1], pre[:, H - 1, W - 1], pre[:, H // 2 + 1, 1] = 0, 0, 0, 0
    x = x.to(BF)
    life = (torch.nn.functional.max_pool2d(x[:, 3:4].float(), 3, 1, 1)[:, 0] > float(np.float32(0.1))) & pre.bool()
    for b in range(B):          # guard: both kinds of cell in every image, and both sides of the clamp
        assert bool(life[b].any()) and bool((~life[b]).any())
        assert float(x[b][:, life[b]].float().max()) > 10.0 and float(x[b][:, life[b]].float().min()) < -10.0
    return x.to(DEV), pre.to(DEV)


@pytest.mark.parametrize("B,C,H,W", [(1, 20, 16, 16), (2, 16, 6, 12), (1, 20, 24, 40)])
def test_cond_finalize_emit_equals_finalize_then_emit(ops, B, C, H, W):
    gen = torch.Generator().manual_seed(B + C + H + W)
    x0 = _dense_state(B, C, H, W, gen).to(BF)
    goal = (torch.randn(B, C - 4, H, W, generator=gen) * 0.5).to(DEV).to(BF)
    stepped = ops.cond_step(x0, None, goal, None, _weights(ops, C, C, x0), seed=3, step=1)
    cases = [("step",) + stepped + (3,), ("built",) + _built_pending(B, C, H, W, gen) + (3,)]
    cases.append(("all alive", cases[1][1], None, -1))
    for name, x_pend, pre, alive_ch in cases:
        want_x = ops.cond_finalize(x_pend, pre, alive_ch)
        if name == "step":
            assert not torch.equal(want_x, x0)
        for out_dtype, out_format in FORMATS:
            got_x, got_img = ops.cond_finalize_emit(x_pend, pre, alive_ch, out_dtype=out_dtype, out_format=out_format)
            assert _same(got_x, want_x), (name, out_dtype, out_format)
            assert _same(got_img, ops.clip_emit_unit(want_x, out_dtype, out_format)), (name, out_dtype, out_format)
    ops.check_errors()


@pytest.mark.parametrize("B,C,H,W,odd", [(1, 5, 5, 7, False), (2, 4, 6, 10, False), (1, 20, 16, 16, True)])
def test_cond_finalize_emit_cell_by_cell_path(ops, B, C, H, W, odd):
    """The launch outside the clip driver's shapes: W % 4 != 0 (a row's last lane holds fewer than four cells), and states that are
    only 2-byte aligned (odd: views one element into their buffers) -- the cells then travel one by one."""
    gen = torch.Generator().manual_seed(B + C + H + W)
    x_pend, pre = _built_pending(B, C, H, W, gen)
    if odd:
        x_pend = torch.cat([x_pend.new_zeros(1), x_pend.reshape(-1)])[1:].view(B, C, H, W)
        assert x_pend.data_ptr() % 4 == 2 and x_pend.is_contiguous()
    want_x = ops.cond_finalize(x_pend, pre, 3)
    for out_dtype, out_format in FORMATS if H % 2 == 0 and W % 2 == 0 else FORMATS[:2]:
        got_x, got_img = ops.cond_finalize_emit(x_pend, pre, 3, out_dtype=out_dtype, out_format=out_format)
        assert _same(got_x, want_x), (out_dtype, out_format)
        assert _same(got_img, ops.clip_emit_unit(want_x, out_dtype, out_format)), (out_dtype, out_format)
    ops.check_errors()


# ------------------------------------------------------------------ 4. driver, bit for bit
def _hand_loop(ops, x, goal, us, w, k, step_n, seed, step0, fmt, same_goal=False):
    """the loop ncahip_cond_clip_bf16 replaces, over the existing bf16 entry points"""
    imgs = []
    for n in range(goal.shape[0] * k):
        un = None if us is None else us[n * step_n:(n + 1) * step_n]
        x, _, _ = ops.cond_grow(x, step_n, goal[0 if same_goal else n // k], un, w, seed=seed, step0=step0 + n * step_n)
        imgs.append(ops.clip_emit_unit(x, *fmt))
    return torch.stack(imgs), x


@pytest.mark.parametrize("B,C,H,W", [(1, 20, 16, 16), (1, 20, 24, 40), (2, 20, 16, 16), (1, 16, 16, 16)])
def test_cond_clip_bf16_equals_the_hand_loop(ops, B, C, H, W):
    gen = torch.Generator().manual_seed(H + W + C + B)
    Fn, E = 3, C - 4
    x0 = _dense_state(B, C, H, W, gen).to(BF)
    goal = (torch.randn(Fn, B, E, H, W, generator=gen) * 0.5).to(DEV).to(BF)
    w = _weights(ops, C, C, x0)
    guarded = False
    for step_n in (2, 3):               # both ring parities
        for k in (1, 2):
            uf = torch.rand(Fn * k * step_n, B, 1, H, W, generator=gen).to(DEV)
            for masks in ("bits", "philox", "float"):
                us = {"bits": ops.pack_fire_mask(uf, 0.5, "cond"), "philox": None, "float": uf}[masks]
                for fmt in FORMATS[:3]:
                    imgs, xs = ops.cond_clip(x0, goal, us, w, k, step_n, seed=11, step0=5, out_dtype=fmt[0], out_format=fmt[1])
                    ref_i, ref_x = _hand_loop(ops, x0, goal, us, w, k, step_n, 11, 5, fmt)
                    tag = (step_n, k, masks, fmt)
                    assert xs.dtype == BF and _same(imgs, ref_i), tag
                    assert _same(xs, ref_x), tag
                    assert not torch.equal(xs, x0), tag
                    if not guarded:       # the goal of every frame matters: frame 0's goal for all frames gives other images
                        oth_i, _ = _hand_loop(ops, x0, goal, us, w, k, step_n, 11, 5, fmt, same_goal=True)
                        assert torch.equal(oth_i[:k], ref_i[:k]) and not torch.equal(oth_i[k:], ref_i[k:])
                        guarded = True
    with pytest.raises(TypeError):      # a bf16 state needs a bf16 goal
        ops.cond_clip(x0, goal.float(), None, w, 1, 2)
    ops.check_errors()


# ------------------------------------------------------------------ 5. sticky error word
def test_cond_clip_bf16_refuses_on_the_sticky_error_word(ops):
    from ncahip import _capi
    L = _capi.lib()
    B, C, H, W, E, Fn = 1, 20, 16, 16, 16, 2
    gen = torch.Generator().manual_seed(0)
    w = _weights(ops, C, 1, _dense_state(B, C, H, W, gen))
    states = torch.full((4, B, C, H, W), -7.0, device=DEV, dtype=BF)
    states[0] = _dense_state(B, C, H, W, gen).to(BF)
    before = states.clone()
    pre = torch.full((2, B, H, W), 9, device=DEV, dtype=torch.uint8)
    goal = torch.randn(Fn, B, E, H, W, generator=gen).to(DEV).to(BF)
    images = torch.full((Fn, B, 3, H, W), -7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    assert L.ncahip_debug_inject_error(1) == 0
    try:
        rc = L.ncahip_cond_clip_bf16(states.data_ptr(), pre.data_ptr(), goal.data_ptr(), E, images.data_ptr(), _capi.CLIP_F32_NCHW, Fn, 1, 2, None,
                                     w.wp.data_ptr(), w.w1.data_ptr(), w.b1.data_ptr(), w.w2.data_ptr(), w.b2.data_ptr(), w.w3.data_ptr(), B, C, H,
                                     W, 64, 3, 0.1, 0.5, -10.0, 10.0, 0, 0, stream)
        assert rc == _capi.EDEVICE and b"error word" in L.ncahip_last_error()
        torch.cuda.synchronize()
        assert _same(states, before) and bool((images == -7.0).all()) and bool((pre == 9).all())      # nothing was enqueued
    finally:
        assert L.ncahip_check_errors(stream, 1) == _capi.EDEVICE      # reports it once more and clears it
    assert L.ncahip_check_errors(stream, 0) == 0
    ops.check_errors()


# ------------------------------------------------------------------ 6. stylize_clip_conditioned(precision="bf16")
def _model(hidden=16, seed=0, size=16):
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(seed)
    m = ConditionedNCA(target_shape=(3, size, size), num_hidden_channels=hidden)
    with torch.no_grad():
        m.update_net.out[4].weight.mul_(0.3)
    return m.to(DEV)


def _clip_frames(n, H, W, seed, u8=False):
    gen = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (n, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV)
    return torch.rand(n, 3, H, W, generator=gen).to(DEV)


@pytest.mark.parametrize("u8", [False, True])
def test_stylize_bf16_continuation_and_chunking(ops, u8):
    from ncahip import video
    m = _model()
    frames = _clip_frames(4, 16, 16, 7, u8)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(1))
    dt = torch.uint8 if u8 else torch.float32

    def run(parts, per_call, rng):
        m.mask_rng, m._mask_step = rng, 0
        torch.manual_seed(123)
        h, outs = x0, []
        for part in parts:
            imgs, h = video.stylize_clip_conditioned(m, part, step_n=3, steps_per_frame=2, state=h, out_dtype=dt, frames_per_call=per_call,
                                                     precision="bf16")
            assert video.stylize_clip_conditioned.last_path == "clip" and h.dtype == BF
            outs.append(imgs)
        return torch.cat(outs), h, torch.cuda.get_rng_state(), m._mask_step

    for rng in ("torch", "philox"):
        base = run([frames], 8, rng)
        assert base[0].shape == ((8, 16, 16, 3) if u8 else (8, 3, 16, 16)) and base[0].dtype == dt and base[3] == 4 * 2 * 3
        for other in (run([frames[:2], frames[2:]], 8, rng), run([frames], 1, rng), run([frames], 3, rng)):
            assert torch.equal(other[0], base[0]) and _same(other[1], base[1])
            assert torch.equal(other[2], base[2]) and other[3] == base[3]
    ops.check_errors()


def test_stylize_bf16_equals_the_hand_loop_and_seeds(ops):
    """The whole function against the loop of section 4 built from the module's own parameters, masks drawn as ConditionedNCA._draw draws
    them; state=None seeds the grid (the seed cast to bf16), warmup_steps run on frame 0's goal before the first image; the returned
    bf16 state continues the clip losslessly."""
    from ncahip import video
    m = _model(seed=2)
    frames = _clip_frames(3, 16, 16, 9)
    torch.manual_seed(5)
    m._mask_step = 0
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=4, steps_per_frame=1, warmup_steps=6, precision="bf16")
    assert video.stylize_clip_conditioned.last_path == "clip" and imgs.shape == (3, 3, 16, 16) and m._mask_step == 6 + 12 and h.dtype == BF
    end = torch.cuda.get_rng_state()
    torch.manual_seed(5)
    goal = ops.clip_encode(frames.unsqueeze(1), m.encoder, dtype=BF)
    x = m.generate_seed(1, size=16).to(DEV).to(BF)
    w = m._weights(x)
    x, _, _ = ops.cond_grow(x, 6, goal[0], m._draw(x, 6), w)
    want = []
    for f in range(3):
        x, _, _ = ops.cond_grow(x, 4, goal[f], m._draw(x, 4), w)
        want.append(ops.clip_emit_unit(x))
    assert torch.equal(imgs, torch.cat(want)) and _same(h, x) and torch.equal(end, torch.cuda.get_rng_state())
    assert float(imgs.max()) > 0.0        # the seed has grown into the image
    # two calls, the second on the returned state
    torch.manual_seed(5)
    m._mask_step = 0
    i1, h1 = video.stylize_clip_conditioned(m, frames[:2], step_n=4, warmup_steps=6, precision="bf16")
    i2, h2 = video.stylize_clip_conditioned(m, frames[2:], step_n=4, state=h1, precision="bf16")
    assert h1.dtype == BF and torch.equal(torch.cat([i1, i2]), imgs) and _same(h2, h)


def test_stylize_bf16_state_dtypes_and_the_f32_default(ops):
    from ncahip import video
    m = _model(seed=3)
    m.mask_rng, m.mask_seed = "philox", 5
    frames = _clip_frames(2, 16, 16, 11)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(4))

    def run(state, **kw):
        m._mask_step = 0
        out = video.stylize_clip_conditioned(m, frames, step_n=3, state=state, **kw)
        return out + (video.stylize_clip_conditioned.last_path,)

    a, b = run(x0, precision="bf16"), run(x0.to(BF), precision="bf16")          # an fp32 state is rounded once at entry
    assert a[2] == b[2] == "clip" and torch.equal(a[0], b[0]) and _same(a[1], b[1]) and a[1].dtype == BF
    assert not torch.equal(x0.to(BF).float(), x0)                                  # (the rounding was one)
    f, g = run(x0, precision="f32"), run(x0)                                       # 'f32' is the call without the keyword
    assert f[2] == g[2] == "clip" and torch.equal(f[0], g[0]) and torch.equal(f[1], g[1]) and f[1].dtype == torch.float32
    assert not torch.equal(a[0], f[0])
    lb, ln = run(x0.to(BF), precision="f32"), run(x0.to(BF))                       # a bf16 state without the keyword: the loop, as before
    assert lb[2] == ln[2] == "loop" and torch.equal(lb[0], ln[0]) and _same(lb[1], ln[1])
    ops.check_errors()


class _WrappedEncoder(torch.nn.Module):
    """A custom encoder module: not the class the fused kernel covers."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x) * 0.5


def test_stylize_bf16_loop_route(ops):
    from ncahip import video
    from ncahip.nca import ConditionedNCA
    from ncahip.encoder import ImageEncoder
    torch.manual_seed(3)
    m = ConditionedNCA(encoder=_WrappedEncoder(ImageEncoder(16, 3)), target_shape=(3, 16, 16)).to(DEV)
    frames = _clip_frames(2, 16, 16, 4)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(2))
    torch.manual_seed(9)
    m._mask_step = 0
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=3, steps_per_frame=2, state=x0, precision="bf16")
    assert video.stylize_clip_conditioned.last_path == "loop" and h.dtype == BF
    torch.manual_seed(9)
    m._mask_step = 0
    state, want = x0.to(BF), []
    with torch.no_grad():
        for f in range(2):
            for _ in range(2):
                state = m.grow(state, 3, frames[f][None])
                want.append(torch.clamp(state[:, :3].float(), 0.0, 1.0))
    assert torch.equal(imgs, torch.cat(want)) and _same(h, state)
    ops.check_errors()


# ------------------------------------------------------------------ 7. against float64
# Largest absolute image difference against the float64 reference with the kernels' rounding points, measured on the MI355X:
# IMAGE_MEASURED = 0 -- image and state came out bit for bit the reference's (every bf16 rounding of the two steps fell the same way in
# fp32 and in float64 arithmetic).  Four times the measured value, rounded up to a power of two, is therefore no bound at all: it would
# demand bit equality with a float64 reference, which fp32 accumulation does not promise.  The bound is the smallest difference the
# format can show instead: one bf16 ulp of an image value in [0.5, 1), 2^-8 -- a single rounding of a visible channel that falls the
# other way passes, two ulps do not.  (The ceiling was 2^-6: a few such ulps, what a goal element rounded the other way can move.)
IMAGE_MEASURED = 0.0
IMAGE_BOUND = 2.0 ** -8


def test_stylize_bf16_against_float64(ops):
    """One frame, step_n = 2, Philox, a dense state with alive = 1.  Reference: the module's encoder in float64, its output rounded to
    bf16 (O._bf) and padded, two O.cond_step_bf16 steps from the bf16 state, the clamp.  No state or pending state of that trajectory
    sits on the life threshold (asserted), so the comparison is continuous."""
    from ncahip import video
    m = _model(seed=4)
    m.mask_rng, m.mask_seed = "philox", 77
    frames = _clip_frames(1, 16, 16, 21)
    x0 = _dense_state(1, 20, 16, 16, torch.Generator().manual_seed(8))
    prm = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    enc64 = copy.deepcopy(m.encoder).cpu().double()
    with torch.no_grad():
        gpad = O.cond_pad_goal(O._bf(enc64(frames.cpu().double())), 20)
    x = O._bf(x0.cpu().double())
    for t in range(2):
        u = torch.from_numpy(np.asarray(O.philox_uniform(77, t, 1, 16, 16))).reshape(1, 1, 16, 16)
        nxt, _, pend = O.cond_step_bf16(x, gpad, u, prm, 3)
        assert not bool(near_threshold(x).any()) and not bool(near_threshold(pend).any()), t
        x = nxt
    assert not bool(near_threshold(x).any())
    ref64 = torch.clamp(x[:, :3], 0.0, 1.0)
    m._mask_step = 0
    imgs, h = video.stylize_clip_conditioned(m, frames, step_n=2, state=x0, precision="bf16")
    assert video.stylize_clip_conditioned.last_path == "clip" and m._mask_step == 2
    m._mask_step = 0
    imgs32, _ = video.stylize_clip_conditioned(m, frames, step_n=2, state=x0, precision="f32")
    err = float((imgs.double().cpu() - ref64).abs().max())
    err_state = float((h.double().cpu() - x).abs().max())
    print(f"stylize_clip_conditioned(precision='bf16') vs float64 with bf16 roundings: image max abs {err:.4e} (bound {IMAGE_BOUND:.4e}, "
          f"measured {IMAGE_MEASURED}), state max abs {err_state:.4e}; vs the f32 image {float((imgs - imgs32).abs().max()):.4e}")
    assert err <= IMAGE_BOUND
    assert not torch.equal(imgs, imgs32)                                      # the path really is the other one
    assert float((imgs - x0[:, :3].clamp(0, 1)).abs().max()) > 1e-3           # the steps moved the image
