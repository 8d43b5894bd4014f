"""Host side of the WIDE range of the bf16-MFMA TRAINING mode of DyNCA (include/ncahip.h, "bf16-MFMA training, the WIDE range":
C <= 32, fc <= 256, single-scale; train_precision="bf16_wide").  The contract, the float64 restatement of it and every stage cap are
the ones of test_dynca_train_bf16_host.py, imported unchanged; this file adds the case rows of the wide range -- the smallest shapes
that reach each shape class and form of the sliced backward kernels (csrc/nca_dynca_bwd_bf16_wide.hip) -- their seeds, the
close-to-fp32 literal of those rows, two planted defects of the slice design, and the exports, refusals and Python plumbing of the new
value.  tests/test_gpu_dynca_train_bf16_wide.py holds the kernels to the same rows.  Nothing here needs a GPU.

Seeds.  One input seed per row (200 .. 205 in row order), the cotangent generator is seeded 1000 + seed, as in the parent file.  They
were chosen on the CPU against the reference alone: the fp32 evaluation of the contract passes every stage cap and check_t1 on every
row, and the flagged-gate share stays under FLAG_FRACTION.  If a row changes, re-select its seed the same way; no GPU result enters."""
import ctypes
import os
import re
import types

import pytest
import torch

from oracle import nca_oracle as O
from test_dynca_bf16_host import _rb, bf16_inputs
from test_dynca_train_bf16_host import (BITS, RATE, _mats, _nsteps_args, check_dh, check_dy, check_t1, check_two_faults, contract_backward,
                                        contract_history, cpu_stage_outputs, rel_l2, run_stage_checks, stage_step)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, fc, c_cond, H, W, pad) -> the class the FORWARD picks (csrc/nca_dynca_bf16_wide.hip), which the backward's slices must share
ROWS = {
    "c17": (1, 17, 128, 0, 11, 35, "reflect"),          # <32, 128>, any-shape form, one channel in the second tile
    "c32fc96": (1, 32, 96, 3, 16, 32, "circular"),      # <32, 128>, K1S = 33: the conditioning slot alone in the fifth chunk
    "fc144": (1, 16, 144, 3, 11, 35, "replicate"),      # <16, 256>, second slice of 16 units
    "fc256": (1, 12, 256, 0, 16, 32, "constant"),       # <16, 256>, padded channels, two full slices
    "c20": (1, 20, 160, 2, 11, 35, "replicate"),        # <32, 256>, the reference's width
    "c32fc256": (2, 32, 256, 3, 24, 40, "circular"),    # the whole class, 12 tiles: the per-workgroup partial reduction
}
SEEDS = {row: 200 + i for i, row in enumerate(ROWS)}
NARROW_ROW = (1, 12, 96, 3, 16, 16, "circular")         # inside the narrow range: the wide entry points run the narrow kernels
# close-to-fp32 literal of the wide rows: twice the worst relative L2 distance of the contract's gradients from the exact float64
# gradients of the same history (T = 3), the margin and rationale of the parent file's CLOSE_TO_F32 (the GPU's accumulation order
# differs from the float64 evaluation's).  Measured values: test_distance_of_the_contract_from_the_exact_gradients.
CLOSE_TO_F32_WIDE = 2 * 0.0788      # worst: b1 of row c32fc96, 7.88e-2


def make_case(row, T=3, device="cpu", dims=None, seed=None):
    """inputs of one case row, the dict of the parent file's make_case: prm, x, cond, us [T,B,1,H,W], g_final, g_states [T+1,...]"""
    B, C, fc, cc, H, W, pad = ROWS[row] if dims is None else dims
    seed = SEEDS[row] if seed is None else seed
    prm, x, cond, _ = bf16_inputs(C, fc, cc, B, H, W, seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    us = torch.rand(T, B, 1, H, W, generator=g)
    g_final = torch.randn(B, C, H, W, generator=g)
    g_states = torch.randn(T + 1, B, C, H, W, generator=g) * 0.3
    g_states[T] = 0
    mv = lambda t: None if t is None else t.to(device)             # noqa: E731
    return dict(prm={k: v.to(device) for k, v in prm.items()}, x=mv(x), cond=mv(cond), us=mv(us), g_final=mv(g_final), g_states=mv(g_states),
                pad=pad, scales=(0,), dims=(B, C, fc, cc, H, W))


def forward_class(C, fc):
    """the class the wide forward picks for a shape outside the narrow range (nca_launch_dynca_step_fwd_bf16_wide)"""
    return (32, 128) if fc <= 128 else ((16, 256) if C <= 16 else (32, 256))


def test_rows_reach_every_class():
    assert {forward_class(*ROWS[r][1:3]) for r in ROWS} == {(32, 128), (16, 256), (32, 256)}
    for r, (B, C, fc, cc, H, W, pad) in ROWS.items():
        assert (C > 16 or fc > 128) and C <= 32 and fc <= 256, r
    assert any(ROWS[r][5] % 4 for r in ROWS) and any(ROWS[r][3] == 0 for r in ROWS)      # any-shape form; no conditioning


# ------------------------------------------------------------------ the reference alone is inside every cap
@pytest.mark.parametrize("row", list(ROWS))
def test_reference_alone_is_inside_every_stage_cap(row):
    """the contract in fp32 (CPU) against the float64 stage references at every wide row and its seed (flagged share asserted inside)"""
    c = make_case(row)
    run_stage_checks(cpu_stage_outputs(c), c)


@pytest.mark.parametrize("row", list(ROWS))
def test_reference_alone_is_inside_the_t1_tolerance(row):
    c = make_case(row, 1)
    got = contract_backward(c["x"][None], c["g_final"], c["g_states"][:1], c["cond"], c["us"][:1], c["prm"], c["pad"], c["scales"],
                            dtype=torch.float32)
    check_t1(got, c, f"contract fp32 {row}")


@pytest.mark.parametrize("row", list(ROWS))
def test_distance_of_the_contract_from_the_exact_gradients(row):
    """relative L2 distance, per gradient tensor, of the contract's gradients (mode-1 history) from the exact float64 gradients of the
    SAME history, T = 3 with g_states; CLOSE_TO_F32_WIDE is twice the worst.  Measured (x0 / w1 / b1 / w2 / b2):
        c17      5.71e-2 5.58e-2 5.85e-2 4.17e-2 5.54e-2      c32fc96  7.63e-2 6.91e-2 7.88e-2 5.17e-2 7.47e-2
        fc144    5.66e-2 6.41e-2 6.41e-2 4.18e-2 4.44e-2      fc256    5.41e-2 4.27e-2 5.19e-2 2.70e-2 3.63e-2
        c20      6.32e-2 4.72e-2 7.56e-2 3.39e-2 6.53e-2      c32fc256 6.16e-2 5.20e-2 7.76e-2 3.46e-2 6.17e-2"""
    c = make_case(row)
    hist = contract_history(c, 3)
    got = contract_backward(hist, c["g_final"], c["g_states"], c["cond"], c["us"], c["prm"], c["pad"], c["scales"])
    ref = contract_backward(hist, c["g_final"], c["g_states"], c["cond"], c["us"], c["prm"], c["pad"], c["scales"], rb=lambda t: t)
    e = {k: rel_l2(got[k], ref[k]) for k in ("x0", "w1", "b1", "w2", "b2")}
    print(f"{row}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e.values()) * 2 <= CLOSE_TO_F32_WIDE, e
    assert max(e.values()) > 1e-4            # the mode does round: the literal is not vacuous


def test_stage_caps_catch_planted_defects_of_the_slice_design():
    """a dropped second hidden slice in W1b^T dhb; and the gate of a <16, 256> case taken from a1 of its CP = 32 zero-padded copy whose
    perception operand holds other bits (truncated instead of rounded to nearest) -- the slices must form a1 from the forward's own
    operands at the forward's class"""
    c = make_case("fc256")
    B, C, fc, cc, H, W = c["dims"]
    good = cpu_stage_outputs(c)
    # 1. dL/dy without the hidden units of the second slice
    w1b = _rb(c["prm"]["w1.weight"][:, :4 * C, 0, 0]).clone()
    w1b[128:] = 0
    with pytest.raises(AssertionError):
        check_dy(torch.einsum("jk,bjhw->bkhw", w1b, good["dh"]), good["dh"], c["prm"], C, "dropped second slice")
    # 2. the gate from a CP = 32 padding fed other bits
    c = make_case("fc144")
    B, C, fc, cc, H, W = c["dims"]
    w1, b1, _ = _mats(c["prm"], torch.float32)
    y = O.dynca_perceive_multiscale(c["x"], c["pad"], (0,), c["cond"])
    trunc = lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32)          # noqa: E731
    ypad = torch.zeros(B, 4 * 32 + cc, H, W)
    w1pad = torch.zeros(fc, 4 * 32 + cc)
    for f in range(4):                                   # blocked [x|Sx|Sy|L] at 32 channel slots, the padding slots zero
        ypad[:, 32 * f:32 * f + C] = trunc(y[:, C * f:C * (f + 1)])
        w1pad[:, 32 * f:32 * f + C] = _rb(w1[:, C * f:C * (f + 1)])
    ypad[:, 128:] = _rb(y[:, 4 * C:])
    w1pad[:, 128:] = _rb(w1[:, 4 * C:])
    other_a1 = torch.einsum("jk,bkhw->bjhw", w1pad, ypad) + b1[None, :, None, None]
    bad = cpu_stage_outputs(c, gate_from=other_a1)
    with pytest.raises(AssertionError):
        check_dh(bad["dh"], bad["y"], c["g_final"], c["cond"], c["us"][0], c["prm"], "gate from a CP = 32 padding with other bits")
    good = cpu_stage_outputs(c)
    check_dh(good["dh"], good["y"], c["g_final"], c["cond"], c["us"][0], c["prm"], "the contract's own gate")


# ------------------------------------------------------------------ exports, refusals, workspace queries
NEW = ["ncahip_dynca_step_bwd_bfmma_wide_workspace", "ncahip_dynca_step_bwd_bfmma_wide_f32", "ncahip_gram_rows_bf16_wide_workspace",
       "ncahip_gram_rows_bf16_wide", "ncahip_dynca_nsteps_bwd_bfmma_wide_workspace", "ncahip_dynca_nsteps_bwd_bfmma_wide_f32"]


def test_exports_are_in_header_library_and_binding():
    from ncahip import _capi
    header = open(os.path.join(ROOT, "include", "ncahip.h")).read()
    dll = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert re.search(r"^(int|size_t)\s+" + name + r"\s*\(", header, re.M), name
        assert name in _capi.SIGNATURES and hasattr(dll, name), name
        if name.endswith("_workspace"):
            assert getattr(_capi.lib(), name).restype is ctypes.c_size_t, name
    assert _capi.version() == 300
    assert "16x16x16_bf16" in header and "WIDE range" in header


def test_driver_refusals_before_any_launch():
    from ncahip import _capi
    L = _capi.lib()
    fn, wsq = L.ncahip_dynca_nsteps_bwd_bfmma_wide_f32, L.ncahip_dynca_nsteps_bwd_bfmma_wide_workspace
    msg = lambda: L.ncahip_last_error().decode()                    # noqa: E731
    wide = dict(C=20, fc=160)
    for shape in (wide, dict(C=12, fc=96)):
        for null in ("states", "g_final", "g_x0", "workspace"):
            assert fn(*_nsteps_args(False, **shape, **{null: True})) == _capi.EINVAL and msg(), null
        assert fn(*_nsteps_args(False, T=0, **shape)) == _capi.EINVAL and "T < 1" in msg()
        need = wsq(1, shape["C"], 16, 16, shape["fc"], 0)
        assert need > 0
        assert fn(*_nsteps_args(False, nbytes=need - 1, **shape)) == _capi.EINVAL and "workspace too small" in msg()
        assert fn(*_nsteps_args(False, ws=0x10004, **shape)) == _capi.ERANGE and "aligned" in msg()
        assert fn(*_nsteps_args(False, ptr=0x5000, **shape)) == _capi.EINVAL and "alias" in msg()          # states == g_x0
        assert L.ncahip_dynca_direction(0x2000, 1, 16, 16) == 0
        try:
            assert fn(*_nsteps_args(False, **shape)) == _capi.EINVAL and "direction field" in msg()
        finally:
            assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0
    assert fn(*_nsteps_args(False, C=33)) == _capi.ERANGE and msg()
    assert fn(*_nsteps_args(False, C=20, fc=257)) == _capi.ERANGE and "wide" in msg()
    # the narrow entry point refuses the wide shapes as it did
    assert L.ncahip_dynca_nsteps_bwd_bfmma_f32(*_nsteps_args(False, C=20)) == _capi.ERANGE
    assert L.ncahip_dynca_nsteps_bwd_bfmma_f32(*_nsteps_args(False, fc=256)) == _capi.ERANGE


def test_stage_entry_refusals_before_any_launch():
    from ncahip import _capi
    L = _capi.lib()
    msg = lambda: L.ncahip_last_error().decode()                    # noqa: E731
    p = 0x1000

    def step(C=20, fc=160, nbytes=1 << 30, ws=0x10000, y=p, g_next=p, g_x=0x3000, fn=L.ncahip_dynca_step_bwd_bfmma_wide_f32):
        return fn(p, None, p, p, p, p, p, 1, C, 16, 16, fc, 0, 1, 0.5, 0, 0, g_next, g_x, y, p, p, p, 0, ws, nbytes, None)
    for shape in (dict(), dict(C=12, fc=96), dict(C=12, fc=256), dict(C=32, fc=96)):
        assert step(y=None, **shape) == _capi.EINVAL and "null" in msg()
        assert step(g_next=None, **shape) == _capi.EINVAL
        assert step(ws=None, **shape) == _capi.EINVAL
        C, fc = shape.get("C", 20), shape.get("fc", 160)
        assert step(nbytes=L.ncahip_dynca_step_bwd_bfmma_wide_workspace(1, C, 16, 16, fc) - 1, **shape) == _capi.EINVAL and "workspace too small" in msg()
        assert step(ws=0x10002, **shape) == _capi.ERANGE and "misaligned" in msg()
        assert step(g_x=p, **shape) == _capi.EINVAL and "alias" in msg()
        assert L.ncahip_dynca_direction(0x2000, 1, 16, 16) == 0
        try:
            assert step(**shape) == _capi.EINVAL and "direction field" in msg()
        finally:
            assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0
    assert step(C=33) == _capi.ERANGE and "C=33" in msg()
    assert step(fc=257) == _capi.ERANGE
    assert step(fn=L.ncahip_dynca_step_bwd_bfmma_f32) == _capi.ERANGE and step(C=12, fc=256, fn=L.ncahip_dynca_step_bwd_bfmma_f32) == _capi.ERANGE

    def gram(a=p, ma=160, nb1=80, b2=p, nb2=2, out=p, ws=0x10000, nbytes=1 << 30):
        return L.ncahip_gram_rows_bf16_wide(a, ma, p, nb1, b2, nb2, 1, 256, out, 0, ws, nbytes, None)
    assert gram(a=None) == _capi.EINVAL and gram(out=None) == _capi.EINVAL and gram(ws=None) == _capi.EINVAL
    assert gram(b2=None) == _capi.EINVAL                             # nb2 > 0 without its tensor
    assert gram(ma=257) == _capi.ERANGE and gram(nb1=131) == _capi.ERANGE
    assert gram(nbytes=L.ncahip_gram_rows_bf16_wide_workspace(160, 82, 1, 256) - 1) == _capi.EINVAL and "workspace too small" in msg()
    assert gram(ws=0x10002) == _capi.ERANGE
    # the old entry keeps its refusals
    assert L.ncahip_gram_rows_bf16(p, 129, p, 48, p, 3, 1, 256, p, 0, 0x10000, 1 << 30, None) == _capi.ERANGE
    assert L.ncahip_gram_rows_bf16(p, 96, p, 80, None, 0, 1, 256, p, 0, 0x10000, 1 << 30, None) == _capi.ERANGE


def test_workspace_queries_are_host_arithmetic():
    """0 outside the wide range, positive and monotone in B inside it, the narrow range's figures inside the narrow range, and less
    scratch than the exact driver at BASELINE configs[4]'s shape"""
    from ncahip import _capi
    L = _capi.lib()
    q = L.ncahip_dynca_nsteps_bwd_bfmma_wide_workspace
    assert q(1, 33, 16, 16, 96, 3) == 0 and q(1, 12, 16, 16, 257, 3) == 0 and q(0, 20, 16, 16, 160, 3) == 0 and q(1, 20, 16, 16, 0, 3) == 0
    for C, fc in [(20, 160), (32, 256), (16, 256), (32, 96)]:
        sizes = [q(B, C, 64, 64, fc, 3) for B in (1, 2, 4, 8, 64)]
        assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    assert q(2, 12, 64, 64, 96, 3) == L.ncahip_dynca_nsteps_bwd_bfmma_workspace(2, 12, 64, 64, 96, 3)
    qs = L.ncahip_dynca_step_bwd_bfmma_wide_workspace
    assert qs(1, 33, 16, 16, 96) == 0 and qs(1, 16, 16, 16, 257) == 0
    s = [qs(B, 32, 64, 64, 256) for B in (1, 2, 4, 8)]
    assert s[0] > 0 and s == sorted(s), s
    assert qs(2, 16, 64, 64, 128) == L.ncahip_dynca_step_bwd_bfmma_workspace(2, 16, 64, 64, 128)
    qg = L.ncahip_gram_rows_bf16_wide_workspace
    assert qg(257, 51, 1, 256) == 0 and qg(96, 133, 1, 256) == 0 and qg(0, 51, 1, 256) == 0
    s = [qg(256, 131, B, 4096) for B in (1, 2, 4, 8)]
    assert s[0] > 0 and s == sorted(s), s
    assert qg(96, 51, 2, 256) == L.ncahip_gram_rows_bf16_workspace(96, 51, 2, 256)
    assert q(4, 32, 512, 512, 256, 3) < L.ncahip_dynca_nsteps_bwd_workspace(4, 32, 512, 512, 256, 3)


# ------------------------------------------------------------------ precedence: two faults in one call
# The wide entry points under the cases and the caller of test_dynca_train_bf16_host.py ("precedence: two faults in one call"), at a
# wide shape and at a narrow one: there they answer with the narrow entry points' checks and messages.  Literals recorded the same way.
TWO_FAULTS = [
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'direction+null', dict(direction=True, states=True),
     (-1, 'dynca nsteps bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'null+C33', dict(states=True, C=33),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'T0+range', dict(T=0, C=20, fc=257),
     (-1, 'dynca nsteps bwd: null pointer or T < 1')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'range+alias', dict(ptr=0x5000, C=20, fc=257),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'alias+short', dict(ptr=0x5000, nbytes=16),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'short+misaligned', dict(nbytes=16, ws=0x10004),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', '4GiB+range', dict(H=4096, W=4096, C=20, fc=257),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca nsteps bwd: 4C*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'alias+short@C20fc160', dict(ptr=0x5000, nbytes=16, C=20, fc=160),
     (-1, 'dynca step: x_in and x_out must not alias (halo reads)')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'short+misaligned@C20fc160', dict(nbytes=16, ws=0x10004, C=20, fc=160),
     (-1, 'dynca nsteps bwd: workspace too small')),
    ('ncahip_dynca_nsteps_bwd_bfmma_wide_f32', 'bits+short@C20fc160', dict(nbytes=16, rate=1.0, seed=BITS, C=20, fc=160),
     (-2, 'bit-packed fire masks (DyNCA): 0 <= update_rate < 1 required (floor(u + rate) must be 0 or 1)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'direction+null', dict(direction=True, g_next=None, C=20, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'null+C33', dict(g_next=None, C=33, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: null pointer')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'range+alias', dict(g_next=0x3000, C=20, fc=257),
     (-2, 'dynca step: C=20 fc=257 c_cond=0 exceeds (32,256,4)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'alias+4GiB', dict(g_next=0x3000, H=4096, W=4096, C=20, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'alias+short', dict(g_next=0x3000, nbytes=16, C=20, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'short+misaligned', dict(nbytes=16, ws=0x10002, C=20, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'misaligned', dict(ws=0x10002, C=20, fc=160),
     (-2, 'dynca step bwd_bfmma_wide: misaligned workspace (4 bytes) or bf16 output (2 bytes)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS, C=20, fc=160),
     (-1, 'dynca step bwd_bfmma_wide: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096, C=20, fc=160),
     (-2, 'dynca step bwd_bfmma_wide: fc*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'direction+null@narrow', dict(direction=True, g_next=None),
     (-1, 'dynca step bwd_bfmma: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'null+C33@narrow', dict(g_next=None, C=33),
     (-1, 'dynca step bwd_bfmma_wide: null pointer')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'range+alias@narrow', dict(g_next=0x3000, fc=257),
     (-2, 'dynca step: C=12 fc=257 c_cond=0 exceeds (32,256,4)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'alias+4GiB@narrow', dict(g_next=0x3000, H=4096, W=4096),
     (-1, 'dynca step bwd_bfmma: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'alias+short@narrow', dict(g_next=0x3000, nbytes=16),
     (-1, 'dynca step bwd_bfmma: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'short+misaligned@narrow', dict(nbytes=16, ws=0x10002),
     (-1, 'dynca step bwd_bfmma: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'misaligned@narrow', dict(ws=0x10002),
     (-2, 'dynca step bwd_bfmma: misaligned workspace (4 bytes) or bf16 output (2 bytes)')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', 'bits+short@narrow', dict(nbytes=16, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd_bfmma: workspace too small')),
    ('ncahip_dynca_step_bwd_bfmma_wide_f32', '4GiB+short@narrow', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca step bwd_bfmma: fc*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_gram_rows_bf16_wide', 'null+range', dict(a=None, ma=257, nb1=80),
     (-1, 'gram_rows_bf16_wide: null pointer')),
    ('ncahip_gram_rows_bf16_wide', 'size+range', dict(HW=0, ma=257, nb1=80),
     (-1, 'gram_rows_bf16_wide: bad size')),
    ('ncahip_gram_rows_bf16_wide', 'range+misaligned', dict(ws=0x10002, ma=160, nb1=131),
     (-2, 'gram_rows_bf16_wide: ma=160 nb=134 outside (<=256 x <=132)')),
    ('ncahip_gram_rows_bf16_wide', 'misaligned+short', dict(ws=0x10002, nbytes=16, ma=160, nb1=80),
     (-2, 'gram_rows_bf16_wide: misaligned pointer (bf16: 2 bytes; fp32 and workspace: 4 bytes)')),
]


@pytest.mark.parametrize("entry,faults,call,want", TWO_FAULTS, ids=[f"{e[7:]}-{f}" for e, f, _, _ in TWO_FAULTS])
def test_the_first_of_two_faults_is_reported(entry, faults, call, want):
    check_two_faults(entry, faults, call, want)


# ------------------------------------------------------------------ Python plumbing without a device
def _model(kind="edge", C=12, fc=96, scales=(0,)):
    from ncahip.models import dynca, dynca_extra
    cls = dynca.DyNCA if kind == "edge" else dynca_extra.DyNCA
    return cls(C, 3, fc_dim=fc, perception_scales=list(scales), device=torch.device("cpu"))


@pytest.mark.parametrize("kind", ["edge", "extra"])
def test_train_precision_accepts_bf16_wide(kind):
    m = _model(kind)
    assert "bf16_wide" in type(m).TRAIN_PRECISIONS
    m.train_precision = "bf16_wide"
    assert m.train_precision == "bf16_wide"
    with pytest.raises(ValueError):
        m.train_precision = "bf16_wider"
    assert m.train_precision == "bf16_wide"


def test_autograd_records_the_effective_precision():
    """the table of the effective precision, through the cfg the autograd function would record"""
    from ncahip import autograd
    seen = {}

    class _Stop(Exception):
        pass

    def fake_apply(x, cond, w1, b1, w2, b2, cfg):
        seen.update(cfg)
        raise _Stop

    real = autograd._DyncaNSteps.apply
    autograd._DyncaNSteps.apply = staticmethod(fake_apply)
    try:
        for C, fc, want, eff in [(12, 96, "bf16_wide", "bf16"), (16, 128, "bf16_wide", "bf16"), (20, 160, "bf16_wide", "bf16_wide"),
                                 (16, 256, "bf16_wide", "bf16_wide"), (32, 96, "bf16_wide", "bf16_wide"), (32, 256, "bf16_wide", "bf16_wide"),
                                 (20, 160, "bf16", "f32"), (12, 256, "bf16", "f32"), (20, 160, "f32", "f32"), (33, 96, "bf16_wide", "f32"),
                                 (33, 96, "bf16", "f32"), (20, 272, "bf16_wide", "f32")]:
            m = _model("edge", C, fc)
            m.train_precision = want
            m.mask_rng = "philox"                    # no draw: nothing here touches a device
            seen.clear()
            with pytest.raises(_Stop):
                autograd.dynca_nsteps_autograd(m, torch.zeros(1, C, 8, 8), None, 2, 0.5)
            assert seen["precision"] == eff, (C, fc, want, seen)
            assert autograd.dynca_train_precision(m, torch.zeros(1, C, 8, 8)) == eff
        two = _model("edge", 20, 160, scales=(0, 1))         # a two-scale wide model runs the composed step: exact
        two.train_precision = "bf16_wide"
        assert autograd.dynca_train_precision(two, torch.zeros(1, 20, 8, 8)) == "f32"
        two = _model("edge", 12, 96, scales=(0, 1))          # a two-scale narrow model: the narrow mode, as with "bf16"
        two.train_precision = "bf16_wide"
        assert autograd.dynca_train_precision(two, torch.zeros(1, 12, 8, 8)) == "bf16"
        for C, fc in [(20, 160), (12, 96)]:                  # a bfloat16 pool where the mode would be selected raises
            m = _model("edge", C, fc)
            m.train_precision = "bf16_wide"
            m.mask_rng = "philox"
            with pytest.raises(ValueError, match="bf16_wide"):
                autograd.dynca_nsteps_autograd(m, torch.zeros(1, C, 8, 8, dtype=torch.bfloat16), None, 2, 0.5)
        out_of_range = _model("edge", 33, 96)
        out_of_range.train_precision = "bf16_wide"
        assert autograd.dynca_train_precision(out_of_range, torch.zeros(1, 33, 8, 8, dtype=torch.bfloat16)) == "f32"
    finally:
        autograd._DyncaNSteps.apply = real


def test_ops_backward_refusals_before_the_device():
    from ncahip import ops
    w = types.SimpleNamespace(fc=160)
    with pytest.raises(ValueError, match="single-scale"):        # two_scale at a wide-only shape
        ops.dynca_nsteps_backward(torch.zeros(2, 1, 20, 8, 8), None, None, w, torch.zeros(1, 20, 8, 8), None, 1, two_scale=True,
                                  precision="bf16_wide")
    with pytest.raises(ValueError):
        ops.dynca_nsteps_backward(torch.zeros(2, 1, 20, 8, 8), None, None, w, torch.zeros(1, 20, 8, 8), None, 1, precision="bf16_wider")


def test_trainer_sets_the_model_attribute():
    from ncahip.dynca_trainer import DyNCATrainer
    m = _model("edge", 20, 160)
    m.seed_mode = "zeros"
    t = DyNCATrainer(m, lambda d: d["nca_state"].sum(), pool_size=4, size=(8, 8), batch_size=2, device=torch.device("cpu"),
                     train_precision="bf16_wide")
    assert t.model.train_precision == "bf16_wide"
