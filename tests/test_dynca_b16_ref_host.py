"""What tests/test_gpu_dynca_b16_ref.py holds the bf16-storage DyNCA step to, checked on the CPU: the bf16 rounding intervals, the
integer round-to-nearest-even, the interval checker against the mistakes it exists to catch, the exact-tie table, and the seed of
the new float64 backward row.

Contract under test (csrc/nca_dynca_step.h, variant DyncaFwdB16): "same kernel, exact f32 compute, round-to-nearest-even on
store".  A stored bf16 value s is the RNE image of every real in [lo(s), hi(s)], lo / hi = the midpoints between s and its lower /
upper bf16 neighbour (max finite: the midpoint to 2^128, where RNE overflows).  The kernel rounds its OWN fp32 result, which may
differ from the float64 reference y64 by util.REPLAY_TOL (the project's bound for one fp32 step from the same input), so
    lo(s) - REPLAY_TOL <= y64 <= hi(s) + REPLAY_TOL            for every element,
and no other number enters.  Where the bf16 half-ulp is far above REPLAY_TOL (|s| > 2^-8 or so) this rejects truncation, a value
one ulp off and every flip whose rounding boundary is farther than REPLAY_TOL from y64.

Run this file directly to regenerate BF16_VJP_SEEDS (python tests/test_dynca_b16_ref_host.py [first_seed [count]])."""
import os
import sys

if __name__ == "__main__":      # the seed search runs without the suite's conftest: the same import paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "video-stylization-with-nca_amd"), os.path.join(_root, "tests")]

import torch

from oracle import nca_oracle as O
from test_gpu_dynca_ref import CASES, TN, bf16_history, make_inputs
from test_gpu_fullsize_ref import DYNCA_GATE_K
from util import REPLAY_TOL

F64 = torch.float64
SAFETY = 4                  # test_gpu_cond_ref.py's convention: the seed search keeps gates SAFETY * DYNCA_GATE_K away
MAX_FINITE = 0x7F7F         # magnitude pattern of the largest finite bf16; 0x7F80 is inf
# (case, pad) -> input seed of the float64 backward row: zero gates within SAFETY * DYNCA_GATE_K on the CPU's bf16 emulation
# (test_gpu_dynca_ref.bf16_history).  The device's stored states differ from the emulation by final-rounding flips; the GPU test
# counts the gates again on those states at DYNCA_GATE_K and asserts zero.
BF16_VJP_SEEDS = {("rem16v", "replicate"): 37370}

# Every row of test_gpu_dynca_ref.CASES with fc <= 128 (the bf16-storage entry points cover no wider hidden layer) and what it
# reaches in nca_launch_dynca_step_fwd_bf16, read off dispatch_dynca / launch_dynca_class with V = DyncaFwdB16
# (csrc/nca_dynca_step.h): the class <CP, FC> is the smallest of <12,96>, <16,128>, <32,128> that covers (C, fc); HAS_COND iff
# c_cond > 0; the VEC form (8-byte groups in pos_load_b16) iff W % 4 == 0 and x_in is 8-byte aligned, else the any-shape form
# (per-element halfwords).  Every slot of a ring buffer torch allocates is 8-byte aligned where W % 4 == 0.
#        id          class      form
ROWS = {"one":      ((12, 96),  "any"),      # 2 x 1 x 1, c_cond 2: every tap of every pad mode lands on the one cell
        "row":      ((12, 96),  "any"),      # 1 x 1 x 5, C = 8: four padded channels, H = 1
        "c5":       ((12, 96),  "any"),      # 3 x 2 x 6, C = 5 without conditioning: the clamp min(ch0 + c, C - 1) holds from channel 5 on
        "h4":       ((12, 96),  "vec"),      # 1 x 4 x 12, no conditioning
        "w8":       ((16, 128), "vec"),      # 1 x 6 x 8
        "band":     ((12, 96),  "vec"),      # 2 x 5 x 12, c_cond 3
        "rem12":    ((12, 96),  "any"),      # 2 x 10 x 34: 2-row and 2-column remainder tiles
        "rem16v":   ((16, 128), "vec"),      # 1 x 18 x 68: 4-column remainder tile, three tile rows
        "c13":      ((16, 128), "vec"),      # 2 x 8 x 32, C = 13: exactly one tile per item, three padded channels
        "fc128":    ((16, 128), "any"),      # 1 x 14 x 30, C = 12 but fc = 128
        "cond4":    ((16, 128), "vec"),      # 1 x 24 x 40, all four conditioning lanes
        "c17":      ((32, 128), "any"),      # 1 x 6 x 10: 15 padded channels above 16
        "c20":      ((32, 128), "vec"),      # 1 x 9 x 36, c_cond 4: 12 padded channels, remainder tiles
        "c32":      ((32, 128), "any"),      # 1 x 10 x 34: the full class
        "c20fc40":  ((32, 128), "any")}      # 1 x 2 x 3, c_cond 1


def b16_class(C, fc):
    """dispatch_dynca<DyncaFwdB16, kDynca12x96, kDynca32x128>"""
    return (12, 96) if C <= 12 and fc <= 96 else (16, 128) if C <= 16 and fc <= 128 else (32, 128) if C <= 32 and fc <= 128 else None


def b16_form(W, addr=0):
    """launch_dynca_class with V::B16"""
    return "vec" if W % 4 == 0 and addr % 8 == 0 else "any"


# ------------------------------------------------------------------------------------ bf16 bit patterns, neighbours, midpoints
def bits_of(s):
    """bf16 tensor -> int64 bit patterns 0 .. 65535"""
    assert s.dtype == torch.bfloat16
    return s.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def from_bits(b):
    """int64 bit patterns -> bf16 tensor"""
    b = b.to(torch.int64) & 0xFFFF
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.bfloat16)


def mag_value(m):
    """float64 value of the magnitude pattern m = 0 .. 0x7F80, exact; 0x7F80 (inf) counts as 2^128, the next value of the grid"""
    m = m.to(torch.int64)
    e, f = m >> 7, (m & 0x7F).to(F64)
    return torch.where(e == 0, torch.ldexp(f, torch.full_like(e, -133)), torch.ldexp(128.0 + f, e - 134))


def interval(s):
    """(lo, hi) float64 of a finite bf16 tensor: the midpoints between each value and its lower / upper bf16 neighbour.  +0 and -0
    are one value: their interval reaches half the smallest subnormal to either side."""
    b = bits_of(s)
    m, neg = b & 0x7FFF, b >= 0x8000
    assert bool((m <= MAX_FINITE).all()), "finite values only"
    v = mag_value(m)
    up = 0.5 * (v + mag_value(m + 1))                                             # exact: both summands have 8-bit significands
    down = torch.where(m == 0, -up, 0.5 * (v + mag_value((m - 1).clamp_min(0))))
    return torch.where(neg, -up, down), torch.where(neg, -down, up)


def rne_bits(y):
    """float64 -> bf16 bit patterns by integer round-to-nearest-even on the float64's own bits, ONE rounding (Tensor.bfloat16() of
    a double rounds twice, through float32); overflow gives inf, NaN is not handled"""
    assert y.dtype == F64
    b = y.contiguous().view(torch.int64)
    sign = (b >> 63) & 1
    e64 = (b >> 52) & 0x7FF
    man = b & ((1 << 52) - 1)
    # normal bf16 (biased exponent e64 - 896 >= 1): exponent and significand in one integer, 45 bits dropped, a carry runs into the exponent
    q = ((e64 - 896) << 52) | man
    normal = (q + ((1 << 44) - 1) + ((q >> 45) & 1)) >> 45
    # bf16 subnormal: (2^52 + man) 2^(e64 - 1075) in units of 2^-133; at a shift of 62 the half exceeds every 53-bit integer
    sh = (942 - e64).clamp(46, 62)
    full = (1 << 52) | man
    sub = (full + ((torch.ones_like(sh) << (sh - 1)) - 1) + ((full >> sh) & 1)) >> sh
    m = torch.where(e64 >= 897, normal, torch.where(e64 == 0, torch.zeros_like(sub), sub)).clamp_max(0x7F80)
    return (sign << 15) | m


def rne_bits_f32(x):
    """float32 -> bf16 bit patterns, the textbook integer form: bits + 0x7FFF + (bit 16), then the upper half"""
    assert x.dtype == torch.float32
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def trunc_bits_f32(x):
    """float32 -> bf16 by dropping the lower half: what a store without rounding would write"""
    return (x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) >> 16


# ------------------------------------------------------------------------------------ the interval checker
def interval_excess(s, y64):
    """per element, how far y64 lies outside the rounding interval of the stored bf16 s (0 inside; NaN stays NaN)"""
    lo, hi = interval(s)
    y64 = y64.to(F64)
    ex = torch.maximum(lo - y64, y64 - hi).clamp_min(0.0)
    return torch.where(torch.isnan(y64), y64, ex)


def interval_check(s, y64, tol=REPLAY_TOL):
    """(bad, worst excess / tol, flips): bad marks every element with not lo - tol <= y64 <= hi + tol (NaN fails); flips counts
    the elements with s != RNE(y64) as values (+0 == -0)"""
    ex = interval_excess(s, y64)
    bad = ~(ex <= tol)
    worst = float("inf") if bool(torch.isnan(ex).any()) else (float(ex.max()) / tol if ex.numel() else 0.0)
    flips = int((from_bits(rne_bits(y64.to(F64))).float() != s.float()).sum())
    return bad, worst, flips


# ------------------------------------------------------------------------------------ the exact-tie case of the GPU file
TIE_C, TIE_FC, TIE_H = 12, 96, 8
TIE_B2 = (2.0 ** -8, -2.0 ** -8, 3 * 2.0 ** -8, -3 * 2.0 ** -8, 2.0 ** -8 + 2.0 ** -16, 2.0 ** -8 - 2.0 ** -16)


def tie_case(W):
    """(x [1,12,8,W] bf16, b2 [12] float32, want [1,12,8,W] int64 bf16 bit patterns, j [1,12,8,W]) of the step x + b2 (w2 = 0,
    every cell fires).  Cell i of channel c holds sign * (1 + j 2^-7) with k = (i + 37 c) % 256, j = k % 128, sign = + for k < 128:
    odd and even j and both signs on every channel.  b2[c] = TIE_B2[c % 6]: +-2^-8 is an exact tie wherever it moves x away from or
    across no binade edge, +-3 2^-8 a tie one step on, 2^-8 +- 2^-16 lie just off the tie.  The exact sum needs 17 significand bits:
    it is a float32, the kernel's own addition does not round, and `want` is the integer RNE of that float32."""
    i = torch.arange(TIE_H * W).reshape(1, 1, TIE_H, W)
    k = (i + 37 * torch.arange(TIE_C).reshape(1, TIE_C, 1, 1)) % 256
    j = k % 128
    x64 = torch.where(k < 128, 1.0, -1.0).to(F64) * (1.0 + j.to(F64) / 128.0)
    b2 = torch.tensor([TIE_B2[c % len(TIE_B2)] for c in range(TIE_C)], dtype=F64)
    total = x64 + b2.reshape(1, TIE_C, 1, 1)
    assert torch.equal(x64.bfloat16().double(), x64) and torch.equal(total.float().double(), total) and torch.equal(b2.float().double(), b2)
    return x64.bfloat16(), b2.float(), rne_bits_f32(total.float()), j


# ------------------------------------------------------------------------------------ the seed of the float64 backward row
def gates_on_emulation(case, pad, seed, k=SAFETY * DYNCA_GATE_K, rate=0.5):
    """hidden pre-activations of updated cells within k (relative) of zero, one step from each state of the CPU's float64 bf16
    emulation (every stored state rounded to bf16); stops at the first step that has one"""
    prm, x0, cond, us, _ = make_inputs(case, seed, device="cpu")
    p64 = {n: v.double() for n, v in prm.items()}
    c64 = None if cond is None else cond.double()
    x, n = x0.bfloat16(), 0
    with torch.no_grad():
        for t in range(TN):
            n += int(O.dynca_gate_influence(x.double(), c64, [us[t]], p64, pad, k, rate)[1].sum())
            if n:
                break
            x = O.dynca_step(x.double(), c64, us[t], p64, pad, rate).float().bfloat16()      # bf16_history's store, step by step
    return n


def search(first, count, case="rem16v", pad="replicate"):
    """prints every qualifying seed in [first, first + count)"""
    for seed in range(first, first + count):
        if gates_on_emulation(case, pad, seed) == 0:
            print(f'    ("{case}", "{pad}"): {seed},', flush=True)


# ==================================================================================== 1. patterns, intervals, the integer RNE
def _all_finite():
    b = torch.arange(65536)
    b = b[(b & 0x7FFF) <= MAX_FINITE]
    return b, from_bits(b)


def test_bits_round_trip_and_values():
    b = torch.arange(65536)
    s = from_bits(b)
    assert torch.equal(bits_of(s), b)
    fb, fs = _all_finite()
    assert fb.numel() == 2 * (MAX_FINITE + 1)
    v = torch.where(fb >= 0x8000, -1.0, 1.0).to(F64) * mag_value(fb & 0x7FFF)
    assert torch.equal(v, fs.double())                                 # mag_value is the value torch widens the pattern to
    assert float(mag_value(torch.tensor([0x7F80]))) == 2.0 ** 128


def test_every_finite_value_lies_inside_its_interval_and_the_intervals_tile_the_line():
    fb, fs = _all_finite()
    lo, hi = interval(fs)
    v = fs.double()
    assert bool((lo < v).all()) and bool((v < hi).all())
    assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(hi).all())
    # ascending by value: negative patterns downwards, then the positive ones; -0 and +0 share one interval
    order = torch.cat([torch.arange(0x8000 + MAX_FINITE, 0x8000 - 1, -1), torch.arange(0, MAX_FINITE + 1)])
    s = from_bits(order)
    lo, hi = interval(s)
    z = MAX_FINITE                                                     # position of -0; +0 follows it
    assert float(s[z].double()) == 0.0 and float(s[z + 1].double()) == 0.0
    assert float(lo[z]) == float(lo[z + 1]) == -(2.0 ** -134) and float(hi[z]) == float(hi[z + 1]) == 2.0 ** -134
    keep = torch.ones(order.numel(), dtype=torch.bool)
    keep[z] = False
    lo, hi, v = lo[keep], hi[keep], s.double()[keep]
    assert bool((v[1:] > v[:-1]).all())
    assert torch.equal(hi[:-1], lo[1:])                                # no gap and no overlap
    assert float(hi[-1]) == 2.0 ** 128 - 2.0 ** 119 and float(lo[0]) == -float(hi[-1])


def test_integer_rne_over_all_patterns():
    fb, fs = _all_finite()
    v = fs.double()
    assert torch.equal(rne_bits(v), fb)                                # every value rounds to itself, the sign of zero kept
    assert torch.equal(rne_bits_f32(fs.float()), fb)
    lo, hi = interval(fs)
    inf = torch.tensor(float("inf"), dtype=F64)
    pos = fb < 0x8000
    m = fb & 0x7FFF
    even_up = torch.where(m & 1 == 0, m, m + 1)                        # the tie at the upper midpoint of |s| goes to the even pattern
    tie = torch.where(pos, hi, lo)                                     # the midpoint away from zero
    assert torch.equal(rne_bits(tie) & 0x7FFF, even_up)
    assert torch.equal(rne_bits(tie) >> 15, (~pos).to(torch.int64))
    inner = torch.where(pos, torch.nextafter(hi, -inf), torch.nextafter(lo, inf))     # just inside: s itself
    outer = torch.where(pos, torch.nextafter(hi, inf), torch.nextafter(lo, -inf))     # just outside: the neighbour (inf past the largest)
    assert torch.equal(rne_bits(inner), fb)
    assert torch.equal(rne_bits(outer), fb + 1)
    assert int(rne_bits(torch.tensor([2.0 ** 128 - 2.0 ** 119], dtype=F64))) == 0x7F80        # the overflow tie goes to even = inf
    # one rounding: a double just above a bf16 tie that float32 rounds ONTO the tie
    y = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=F64)
    assert int(rne_bits(y)) == 0x3F81 and int(bits_of(y.float().bfloat16())) == 0x3F80
    # float32 inputs: the textbook form, torch's own conversion and the float64 routine agree
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(1)) * torch.logspace(-42, 38, 1 << 16, base=10.0).float()
    x = x[torch.isfinite(x)]
    assert torch.equal(rne_bits_f32(x), bits_of(x.bfloat16())) and torch.equal(rne_bits(x.double()), rne_bits_f32(x))


# ==================================================================================== 2. the checker catches what it is for
def _sample(n=4096, seed=2):
    g = torch.Generator().manual_seed(seed)
    y = (0.25 + 1.75 * torch.rand(n, generator=g, dtype=F64)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return y                                                           # 0.25 <= |y| < 2: half an ulp is 2^-10 .. 2^-8, far above REPLAY_TOL


def test_checker_accepts_rne():
    y = _sample()
    bad, worst, flips = interval_check(from_bits(rne_bits(y)), y)
    assert not bool(bad.any()) and worst == 0.0 and flips == 0
    y32 = y.float()                                                    # and an fp32 evaluation rounded by torch
    bad, worst, flips = interval_check(y32.bfloat16(), y32.double())
    assert not bool(bad.any()) and worst == 0.0 and flips == 0


def test_checker_accepts_a_flip_across_a_boundary_within_the_tolerance():
    s = from_bits(rne_bits(_sample()))
    lo, hi = interval(s)
    for d in (0.25 * REPLAY_TOL, 0.999 * REPLAY_TOL):
        for y in (hi + d, lo - d):                                     # y64 rounds to the neighbour, the kernel's own fp32 value to s
            bad, worst, flips = interval_check(s, y)
            assert not bool(bad.any()) and flips == s.numel()
            assert abs(worst - d / REPLAY_TOL) < 1e-6


def test_checker_rejects_a_flip_whose_boundary_is_farther_than_the_tolerance():
    s = from_bits(rne_bits(_sample()))
    lo, hi = interval(s)
    for d in (1.001 * REPLAY_TOL, 2 * REPLAY_TOL):
        for y in (hi + d, lo - d):
            bad, worst, flips = interval_check(s, y)
            assert bool(bad.all()) and worst > 1.0 and flips == s.numel()
    y = hi.clone()
    y[7] = float("nan")
    bad, worst, _ = interval_check(s, y)
    assert int(bad.sum()) == 1 and bool(bad[7]) and worst == float("inf")          # NaN fails


def test_checker_rejects_truncation():
    y = _sample().float()
    t = from_bits(trunc_bits_f32(y))
    differs = t.float() != y.bfloat16().float()
    assert 0.4 < float(differs.float().mean()) < 0.6                   # truncation and RNE part ways on the upper half of every ulp
    bad, worst, flips = interval_check(t, y.double())
    assert flips == int(differs.sum())
    assert not bool((bad & ~differs).any())
    # what slips through lies within REPLAY_TOL above a midpoint: REPLAY_TOL / (ulp / 2) of the differing ones, at most 2^10 * 1e-5 = 1 %
    assert int((differs & ~bad).sum()) <= 0.02 * int(differs.sum()) and worst > 10.0


def test_checker_rejects_a_value_one_ulp_off():
    b = rne_bits(_sample())
    y = from_bits(b).double()                                          # the reference in the middle of its interval
    for step in (1, -1):
        bad, worst, flips = interval_check(from_bits(b + step), y)
        assert bool(bad.all()) and flips == y.numel()
        assert worst >= 2.0 ** -11 / REPLAY_TOL                        # at least half the ulp below 0.25 outside


def test_zero_sign_counts_as_no_flip():
    y = torch.zeros(4, dtype=F64)
    s = from_bits(torch.tensor([0x0000, 0x8000, 0x0000, 0x8000]))
    bad, worst, flips = interval_check(s, y)
    assert not bool(bad.any()) and worst == 0.0 and flips == 0


# ==================================================================================== 3. the tie table
def test_tie_table_against_torch():
    for W in (32, 30):
        x, b2, want, j = tie_case(W)
        total = x.float() + b2.reshape(1, TIE_C, 1, 1)                 # exact in float32
        assert torch.equal(want, bits_of(total.bfloat16()))
        assert torch.equal(want, rne_bits(x.double() + b2.double().reshape(1, TIE_C, 1, 1)))
        assert bool((bits_of(x) & 0x7FFF != 0).all())                  # no zero, so no -0 among the inputs
        lo, hi = interval(from_bits(want))
        on_tie = (total.double() == lo) | (total.double() == hi)
        trunc = trunc_bits_f32(total)
        for c in range(TIE_C):
            jc, xc = j[0, c], x[0, c].float()
            assert bool((jc % 2 == 0).any()) and bool((jc % 2 == 1).any()) and bool((xc > 0).any()) and bool((xc < 0).any()), (W, c)
            tied = int(on_tie[0, c].sum())
            if c % 6 < 4:      # +-2^-8 and +-3 2^-8: a tie wherever x + b2 stays in [1, 2) in magnitude
                assert tied >= 0.45 * jc.numel(), (W, c, tied)
                assert bool((want[0, c][on_tie[0, c]] & 1 == 0).all())             # every tie went to the even pattern
            else:
                assert tied == 0, (W, c)
            assert bool((trunc[0, c] != want[0, c]).any()), (W, c)     # a truncating store misses every channel
        # j = 127: the tie at 2 - 2^-8 rounds up to +-2.0 (channel 0: +2^-8 on positive x; channel 1: -2^-8 on negative x)
        up = (j[0, 0] == 127) & (x[0, 0].float() > 0)
        dn = (j[0, 1] == 127) & (x[0, 1].float() < 0)
        assert bool(up.any()) and bool(dn.any()), W
        assert bool((want[0, 0][up] == 0x4000).all()) and bool((want[0, 1][dn] == 0xC000).all())


# ==================================================================================== 4. the rows and what they reach
def test_rows_are_the_table_rows_up_to_fc_128_and_reach_every_class_in_both_forms():
    assert list(ROWS) == [c for c in CASES if CASES[c][1] <= 128]
    seen = set()
    for case, (cls, form) in ROWS.items():
        C, fc, cc, B, H, W = CASES[case]
        assert b16_class(C, fc) == cls and b16_form(W) == form, case
        assert (B * C * H * W) % 4 == 0, case                         # what ncahip_dynca_nsteps_bwd_bf16 asks for
        seen.add((cls, form, cc > 0))
    for cls in ((12, 96), (16, 128), (32, 128)):
        for form in ("vec", "any"):
            assert (cls, form, True) in seen, (cls, form)
        assert any((cls, f, False) in seen for f in ("vec", "any")), cls
    assert b16_form(12, addr=2) == "any"                               # a view one element into its buffer at W % 4 == 0


# ==================================================================================== 5. the seed of the float64 backward row
def test_backward_row_seed_qualifies():
    for (case, pad), seed in BF16_VJP_SEEDS.items():
        assert CASES[case][:2] == (16, 128)                            # class <16,128>
        assert gates_on_emulation(case, pad, seed) == 0, (case, pad, seed)
        # the same count on test_gpu_dynca_ref.bf16_history's states, the emulation the two older rows were searched with
        prm, x0, cond, us, _ = make_inputs(case, seed, device="cpu")
        p64 = {n: v.double() for n, v in prm.items()}
        c64 = None if cond is None else cond.double()
        states = bf16_history(p64, x0, cond, us, pad, 0.5)
        assert len(states) == TN + 1 and all(s.dtype == torch.bfloat16 for s in states)
        assert sum(int(O.dynca_gate_influence(states[t].double(), c64, [us[t]], p64, pad, SAFETY * DYNCA_GATE_K, 0.5)[1].sum())
                   for t in range(TN)) == 0
        assert float((us + 0.5).floor().mean()) > 0.4                  # and about half of the cells fire


if __name__ == "__main__":
    torch.set_num_threads(1)
    search(int(sys.argv[1]) if len(sys.argv) > 1 else 36000, int(sys.argv[2]) if len(sys.argv) > 2 else 100000)
