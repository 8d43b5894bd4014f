"""Host side of the opt-in bf16-MFMA DyNCA step (ncahip_dynca_precision, include/ncahip.h): the export and its bindings, the
set / return-previous protocol, the context manager, stylize_clip's argument check -- none of which needs a GPU -- and the REFERENCE
the GPU tests (test_gpu_dynca_bf16.py) compare the kernels with.

The reference is a restatement of the mode's arithmetic contract: perception in float64 (oracle.nca_oracle, read-only), the contract's
roundings through .to(torch.bfloat16) (round to nearest even), both products in float64:

    y  = bf16([perception(x) | cond])          w1, w2 -> bf16 once          b1, b2 unrounded
    h  = bf16(relu(w1 y + b1))                 dx = w2 h + b2               x' = x + dx * floor(u + rate)

Beside the value it returns, per element, the first-order bound

    E = 2^-8 * sum_j |w2_cj| * (|h_j| + sum_k |w1_jk| |y_k|)          (times the fire mask, as the step applies it)

-- the largest change the operand and weight roundings (relative 2^-9 each: y and w1 into the hidden layer, h and w2 into the output),
or a one-ulp (2^-8) rounding flip of every operand, can cause.  Two caps follow from it, used for every kernel of the mode:
  (a) every element within E * (1 + 2^-7) of the restatement;
  (b) at most 0.5 % of the elements off by more than 1e-5 * max(1, |x|): an honest implementation differs from the restatement by
      fp32 accumulation order (1e-6 relative) except where one of its operands sat within that of a bf16 rounding boundary and went
      the other way, which touches the C elements of one cell; a wrong k order, a dropped K chunk or truncation touch nearly all.
      |x| is the magnitude of the element that is compared, i.e. the restatement's x'.  For a state drawn from U(-1, 1) that is
      also the input's magnitude; in the teacher-forced replay it is not: these weight distributions are expansive (max |x| 1, 11,
      57, 193, 772, 2658 over six free-running steps at 12 / 96), a cell's dx is then hundreds while its own input element may be
      ~1, and 1e-5 of the INPUT element is below the fp32 accumulation error of dx itself -- the fp32 CPU evaluation of the
      contract alone then has 0.95 % / 2.3 % of its elements beyond it at steps 4 / 5 (0.08 % / 0.10 % relative to x').
      check_caps prints the input-relative fraction as well.
The last test here evaluates the same contract in fp32 on the CPU and holds it to (a) and (b): the reference alone stays inside."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIP_TOL, FLIP_FRACTION = 1e-5, 0.005


# ------------------------------------------------------------------ the reference
def bf16_inputs(C, fc, c_cond, B, H, W, seed, device="cpu", w_scale=1.0):
    """x ~ U(-1, 1), w1 ~ N(0, 0.15^2), w2 ~ N(0, 0.1^2), tanh'd conditioning, small biases, explicit uniforms; fp32."""
    g = torch.Generator().manual_seed(seed)
    k1 = 4 * C + c_cond
    prm = {"w1.weight": torch.randn(fc, k1, 1, 1, generator=g) * 0.15 * w_scale, "w1.bias": torch.randn(fc, generator=g) * 0.1,
           "w2.weight": torch.randn(C, fc, 1, 1, generator=g) * 0.1 * w_scale, "w2.bias": torch.randn(C, generator=g) * 0.02}
    x = torch.rand(B, C, H, W, generator=g) * 2 - 1
    cond = torch.tanh(torch.randn(B, c_cond, H, W, generator=g) * 2) if c_cond else None
    u = torch.rand(B, 1, H, W, generator=g)
    mv = lambda t: None if t is None else t.to(device)             # noqa: E731
    return {k: v.to(device) for k, v in prm.items()}, mv(x), mv(cond), mv(u)


def _rb(t):
    """the contract's rounding: to bf16 (round to nearest even) and back, in the tensor's own dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def contract_step(x, cond, u, prm, pad, rate=0.5, scales=(0,), dtype=torch.float64, rb=_rb):
    """(x', E) of one step under the contract, everything evaluated in `dtype` (float64: the reference; float32: a second
    evaluation of the same contract, for the self-check below).  u: the fp32 uniforms [B,1,H,W].  rb: the operand rounding."""
    xd = x.to(dtype)
    y = O.dynca_perceive_multiscale(xd, pad, scales, None if cond is None else cond.to(dtype))
    w1, b1 = prm["w1.weight"].to(dtype)[:, :, 0, 0], prm["w1.bias"].to(dtype)
    w2, b2 = prm["w2.weight"].to(dtype)[:, :, 0, 0], prm["w2.bias"].to(dtype)
    h = F.relu(torch.einsum("jk,bkhw->bjhw", rb(w1), rb(y)) + b1[None, :, None, None])
    dx = torch.einsum("cj,bjhw->bchw", rb(w2), rb(h)) + b2[None, :, None, None]
    m = (u.float() + torch.tensor(rate, dtype=torch.float32)).floor().to(dtype)          # floorf(u + rate) in fp32, as the kernels
    e = h.abs() + torch.einsum("jk,bkhw->bjhw", w1.abs(), y.abs())
    E = 2.0 ** -8 * torch.einsum("cj,bjhw->bchw", w2.abs(), e) * m
    return xd + dx * m, E


def check_caps(got, ref, E, x, what=""):
    """(a) and (b) of the module docstring; prints the figures first.  x: the step's input state (for the printed second fraction).
    Returns (worst |d| / E, fraction beyond FLIP_TOL)."""
    d = (got.double() - ref.double()).abs()
    ratio = float((d / E.double().clamp_min(1e-30))[E > 0].max()) if bool((E > 0).any()) else 0.0
    off_mask = float(d[E <= 0].max()) if bool((E <= 0).any()) else 0.0
    frac = float((d > FLIP_TOL * ref.double().abs().clamp_min(1.0)).double().mean())
    frac_in = float((d > FLIP_TOL * x.double().abs().clamp_min(1.0)).double().mean())
    print(f"{what}: max |d| {float(d.max()):.3e}, max |d| / E {ratio:.3e}, where the mask is 0: {off_mask:.1e}, "
          f"beyond {FLIP_TOL:g} * max(1, |x'|): {100 * frac:.3f} % (cap {100 * FLIP_FRACTION:g} %; relative to the input state: "
          f"{100 * frac_in:.3f} %), max |x'| {float(ref.abs().max()):.3g}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((d <= E.double() * (1 + 2.0 ** -7)).all()), (what, ratio, off_mask)
    assert frac <= FLIP_FRACTION, (what, frac)
    return ratio, frac


@pytest.mark.parametrize("C,fc", [(12, 96), (16, 128)])
@pytest.mark.parametrize("scales", [(0,), (0, 1)])
def test_reference_alone_is_inside_the_caps(C, fc, scales):
    """float64 restatement against an fp32 evaluation of the same contract (CPU), the GPU tests' input distributions, 32 x 32"""
    for w_scale in (1.0, 3.0):
        prm, x, cond, u = bf16_inputs(C, fc, 3, 1, 32, 32, seed=100 * C + int(w_scale))
        ref, E = contract_step(x, cond, u, prm, "circular", scales=scales)
        got, _ = contract_step(x, cond, u, prm, "circular", scales=scales, dtype=torch.float32)
        assert float(E.max()) > 1e-4 and float((E > 0).double().mean()) > 0.3            # the bound is not vacuous, about half the cells fire
        check_caps(got, ref, E, x, f"contract fp32 vs float64 C={C} fc={fc} scales={scales} weights x{w_scale:g}")
        # and the contract stays well inside E of the exact fp32 step it approximates
        exact = O.dynca_step(x, cond, u, prm, "circular", 0.5, scales)
        r = float(((ref - exact.double()).abs() / E.clamp_min(1e-30))[E > 0].max())
        print(f"   |contract - exact fp32 step| / E: {r:.3f}")
        assert r < 1.0


def test_caps_catch_truncation_and_a_dropped_chunk():
    """negative controls on the CPU: truncation instead of RNE, and a layer-2 product without its last 32 hidden units, miss (b)"""
    prm, x, cond, u = bf16_inputs(12, 96, 3, 1, 32, 32, seed=7)
    ref, E = contract_step(x, cond, u, prm, "replicate")
    trunc = lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)         # noqa: E731
    bad, _ = contract_step(x, cond, u, prm, "replicate", dtype=torch.float32, rb=trunc)
    with pytest.raises(AssertionError):
        check_caps(bad, ref, E, x, "truncation")
    p2 = dict(prm)
    p2["w2.weight"] = prm["w2.weight"].clone()
    p2["w2.weight"][:, 64:] = 0
    bad, _ = contract_step(x, cond, u, p2, "replicate", dtype=torch.float32)
    with pytest.raises(AssertionError):
        check_caps(bad, ref, E, x, "dropped chunk")


# ------------------------------------------------------------------ the export
def test_export_is_in_header_library_and_binding():
    from ncahip import _capi
    header = open(os.path.join(ROOT, "include", "ncahip.h")).read()
    assert re.search(r"^int\s+ncahip_dynca_precision\s*\(\s*int\s+mode\s*\)\s*;", header, re.M)
    assert _capi.SIGNATURES["ncahip_dynca_precision"] == [ctypes.c_int]
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), "ncahip_dynca_precision")


def test_set_returns_previous_and_rejects_unknown_modes():
    from ncahip import _capi, ops
    L = _capi.lib()
    first = L.ncahip_dynca_precision(0)
    assert first in (0, 1)
    try:
        assert L.ncahip_dynca_precision(1) == 0 and L.ncahip_dynca_precision(1) == 1
        for bad in (2, -1, 7):
            assert L.ncahip_dynca_precision(bad) == _capi.EINVAL
            assert L.ncahip_dynca_precision(1) == 1                       # unchanged by the refused call
        assert L.ncahip_dynca_precision(0) == 1 and L.ncahip_dynca_precision(0) == 0
        assert ops.set_dynca_precision("bf16") == "f32" and ops.set_dynca_precision("f32") == "bf16"
        with pytest.raises(ValueError):
            ops.set_dynca_precision("fp16")
        assert L.ncahip_dynca_precision(0) == 0
    finally:
        L.ncahip_dynca_precision(first)


def test_context_manager_restores_on_exception_and_nests():
    from ncahip import _capi, ops
    mode = lambda: ops.set_dynca_precision(ops.set_dynca_precision("f32"))          # noqa: E731  (reads the mode: set f32, put back)
    L = _capi.lib()
    L.ncahip_dynca_precision(0)
    with ops.dynca_precision("bf16"):
        assert L.ncahip_dynca_precision(1) == 1
        with ops.dynca_precision("f32"):
            assert L.ncahip_dynca_precision(0) == 0
        assert L.ncahip_dynca_precision(1) == 1
    assert L.ncahip_dynca_precision(0) == 0
    with pytest.raises(RuntimeError):
        with ops.dynca_precision("bf16"):
            raise RuntimeError("inside")
    assert L.ncahip_dynca_precision(0) == 0
    with pytest.raises(ValueError):
        with ops.dynca_precision("bogus"):
            pass
    assert mode() == "f32"


def test_bf16_ok_range():
    from ncahip import ops
    assert ops.dynca_bf16_ok(12, 96) and ops.dynca_bf16_ok(16, 128) and ops.dynca_bf16_ok(13, 96) and ops.dynca_bf16_ok(8, 32)
    assert not ops.dynca_bf16_ok(20, 96) and not ops.dynca_bf16_ok(16, 256) and not ops.dynca_bf16_ok(32, 128)


def test_stylize_clip_refuses_an_unknown_precision_before_the_device():
    from ncahip import _capi, video

    class Untouchable:                      # any attribute access fails: the check comes first
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the precision was checked")

    frames = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="precision"):
        video.stylize_clip(Untouchable(), frames, precision="bogus")
    assert _capi.lib().ncahip_dynca_precision(0) == 0
