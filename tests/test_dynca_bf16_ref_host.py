"""What tests/test_gpu_dynca_bf16_ref.py holds the bf16-MFMA DyNCA step (ncahip_dynca_precision mode 1) to, checked on the CPU: the
row tables with the kernel instantiation every row reaches, the literal input seeds, the proof that the comparator is fair on every
(row, pad), and the mistakes the comparator exists to catch.

Comparator, unchanged: test_dynca_bf16_host.py's float64 restatement of the mode's contract (contract_step), its first-order bound E
and check_caps -- (a) every element within E (1 + 2^-7), (b) at most FLIP_FRACTION = 0.5 % of the elements beyond FLIP_TOL.  No
tolerance is introduced here.

Rows.  The geometry (C, fc, c_cond, H, W) comes from the tables the project already maintains: every row of
test_gpu_dynca_ref.CASES with C <= 16 and fc <= 128, every row of test_gpu_two_scale_ref.CASES, plus one added row each
(c14nc / ms14nc) for the class <16,128,false> any-shape that no table row reaches, plus the four rows of the persistent kernels.
What a row reaches, read off launch_dynca_fwd_ladder / dispatch_dynca / launch_dynca_class (csrc/nca_dynca_step.h) with V = DyncaFwdBf or
DyncaFwdMsBf: the class <CP, FC> is <12,96> iff C <= 12 and fc <= 96, else <16,128>; HAS_COND iff c_cond > 0; the VEC form (16-byte
row loads) iff W % 4 == 0 and the first plane is 16-byte aligned, else the any-shape form.  The persistent kernels
(dispatch_persist, csrc/nca_dynca_persist.hip): launch_cfg<MS, CP, FC, HAS_COND, true> with the same class rule, planes of whole
16 x 16 tiles.

Population.  Cap (b) is a fraction and one flipped rounding moves all C elements of a cell, so a row needs cells to count over: the
batch of every table row is raised to B = ceil(1024 / (H W)) (1024 planes for `one`, 1 for `rem16v`).  Tile edges are per plane: the
class a row reaches does not change.  The persistent rows keep the batch their table gives (512 cells each).

Seeds.  One literal seed per (row, pad), chosen on the CPU against the reference alone (python tests/test_dynca_bf16_ref_host.py
prints the table): the fp32 evaluation of the contract must pass check_caps against the float64 restatement with a cap-(b) fraction
of at most HALF of FLIP_FRACTION -- the other half is left to the kernel's different accumulation order --, E.max() > 1e-4 and
between 25 % and 75 % of the cells fire.  No GPU result enters the choice."""
import contextlib
import io
import math
import os
import sys

if __name__ == "__main__":      # the seed search runs without the suite's conftest: the same import paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "video-stylization-with-nca_amd"), os.path.join(_root, "tests")]

import pytest
import torch

import test_gpu_dynca_ref as S1
import test_gpu_two_scale_ref as S2
from oracle import nca_oracle as O
from test_dynca_bf16_host import FLIP_FRACTION, bf16_inputs, check_caps, contract_step

CELLS = 1024                # every table row is batched up to at least this many cells
T_MAX = 4                   # uniforms drawn per (row, pad): three for the replay, four for the longest persistent run
HALF_CAP = FLIP_FRACTION / 2

#                 id        class      HAS_COND form         geometry (C, fc, c_cond, H, W) and what it is for
SINGLE = {"one":    ((12, 96),  True,  "any"),      # 12, 96, 2, 1 x 1: a plane of one cell, every tap of every pad mode lands on it
          "row":    ((12, 96),  True,  "any"),      # 8, 32, 1, 1 x 5: one row, C = 8 (four padded channels), ONE conditioning lane, fc = 32
          "c5":     ((12, 96),  False, "any"),      # 5, 24, 0, 2 x 6: C % 4 != 0 below 12, fc = 24 ends 8 units into the second 16-tile
          "h4":     ((12, 96),  False, "vec"),      # 12, 96, 0, 4 x 12
          "w8":     ((16, 128), True,  "vec"),      # 16, 128, 2, 6 x 8
          "band":   ((12, 96),  True,  "vec"),      # 12, 96, 3, 5 x 12
          "rem12":  ((12, 96),  True,  "any"),      # 12, 96, 3, 10 x 34: 2-row and 2-column remainder tiles
          "rem16v": ((16, 128), True,  "vec"),      # 16, 128, 3, 18 x 68: 4-column remainder tile, three tile rows
          "c13":    ((16, 128), False, "vec"),      # 13, 104, 0, 8 x 32: three padded channels, fc = 104 ends 8 units into the seventh 16-tile
          "fc128":  ((16, 128), True,  "any"),      # 12, 128, 2, 14 x 30
          "cond4":  ((16, 128), True,  "vec"),      # 16, 128, 4, 24 x 40: all four conditioning lanes
          "c14nc":  ((16, 128), False, "any")}      # 14, 100, 0, 3 x 5 (added): fc ends 4 units into a 16-tile, two padded channels
ADDED_SINGLE = {"c14nc": (14, 100, 0, 3, 5)}
TWO = {"c1x1":    ((12, 96),  True,  "any"),        # 12, 96, 2, 2 x 2: coarse grid 1 x 1
       "c2x2":    ((12, 96),  False, "vec"),        # 12, 96, 0, 4 x 4
       "c5":      ((12, 96),  False, "any"),        # 5, 24, 0, 2 x 6
       "odd3x5":  ((12, 96),  True,  "any"),        # 8, 40, 1, 6 x 10: fc = 40 ends 8 units into the third 16-tile, one conditioning lane
       "rem12":   ((12, 96),  True,  "any"),        # 12, 96, 3, 10 x 34
       "rem16":   ((16, 128), True,  "any"),        # 16, 128, 3, 18 x 66: W = 2 (mod 4)
       "c13":     ((16, 128), False, "vec"),        # 13, 104, 0, 8 x 32
       "fc128":   ((16, 128), True,  "any"),        # 12, 128, 2, 14 x 30
       "cond4":   ((16, 128), True,  "vec"),        # 16, 128, 4, 24 x 40
       "persist": ((12, 96),  True,  "vec"),        # 12, 96, 2, 16 x 64
       "ms14nc":  ((16, 128), False, "any")}        # 14, 100, 0, 6 x 10 (added)
ADDED_TWO = {"ms14nc": (14, 100, 0, 6, 10)}
# the persistent kernels: (C, fc, c_cond, B, H, W), run single- and two-scale, so all eight launch_cfg<MS, CP, FC, HAS_COND, true> run
#                 id      geometry                    class      HAS_COND
PERSIST = {"p12":  ((12, 96, 3, 1, 16, 32),  (12, 96),  True),
           "p5":   ((5, 24, 0, 2, 16, 16),   (12, 96),  False),    # B = 2, C % 4 != 0, a partial hidden tile
           "p16":  ((16, 128, 4, 1, 32, 16), (16, 128), True),     # all four conditioning lanes
           "p13":  ((13, 104, 0, 1, 16, 32), (16, 128), False)}

# ---- (two_scale, row, pad) -> input seed: see the module docstring; regenerate with python tests/test_dynca_bf16_ref_host.py ----
SEEDS = {
    (False, "one", "constant"): 50000,
    (False, "one", "replicate"): 50100,
    (False, "one", "circular"): 50200,
    (False, "row", "constant"): 50300,
    (False, "row", "replicate"): 50400,
    (False, "row", "circular"): 50500,
    (False, "c5", "constant"): 50600,
    (False, "c5", "replicate"): 50700,
    (False, "c5", "circular"): 50800,
    (False, "c5", "reflect"): 50900,
    (False, "h4", "constant"): 51000,
    (False, "h4", "replicate"): 51100,
    (False, "h4", "circular"): 51200,
    (False, "h4", "reflect"): 51300,
    (False, "w8", "constant"): 51400,
    (False, "w8", "replicate"): 51500,
    (False, "w8", "circular"): 51600,
    (False, "w8", "reflect"): 51700,
    (False, "band", "constant"): 51800,
    (False, "band", "replicate"): 51900,
    (False, "band", "circular"): 52000,
    (False, "band", "reflect"): 52100,
    (False, "rem12", "constant"): 52200,
    (False, "rem12", "replicate"): 52300,
    (False, "rem12", "circular"): 52400,
    (False, "rem12", "reflect"): 52500,
    (False, "rem16v", "constant"): 52600,
    (False, "rem16v", "replicate"): 52700,
    (False, "rem16v", "circular"): 52800,
    (False, "rem16v", "reflect"): 52900,
    (False, "c13", "constant"): 53000,
    (False, "c13", "replicate"): 53100,
    (False, "c13", "circular"): 53200,
    (False, "c13", "reflect"): 53300,
    (False, "fc128", "constant"): 53400,
    (False, "fc128", "replicate"): 53500,
    (False, "fc128", "circular"): 53600,
    (False, "fc128", "reflect"): 53700,
    (False, "cond4", "constant"): 53800,
    (False, "cond4", "replicate"): 53900,
    (False, "cond4", "circular"): 54000,
    (False, "cond4", "reflect"): 54100,
    (False, "c14nc", "constant"): 54200,
    (False, "c14nc", "replicate"): 54300,
    (False, "c14nc", "circular"): 54400,
    (False, "c14nc", "reflect"): 54500,
    (True, "c1x1", "constant"): 54600,
    (True, "c1x1", "replicate"): 54700,
    (True, "c1x1", "circular"): 54800,
    (True, "c2x2", "constant"): 54900,
    (True, "c2x2", "replicate"): 55000,
    (True, "c2x2", "circular"): 55100,
    (True, "c2x2", "reflect"): 55200,
    (True, "c5", "constant"): 55300,
    (True, "c5", "replicate"): 55400,
    (True, "c5", "circular"): 55500,
    (True, "odd3x5", "constant"): 55600,
    (True, "odd3x5", "replicate"): 55700,
    (True, "odd3x5", "circular"): 55800,
    (True, "odd3x5", "reflect"): 55900,
    (True, "rem12", "constant"): 56000,
    (True, "rem12", "replicate"): 56100,
    (True, "rem12", "circular"): 56200,
    (True, "rem12", "reflect"): 56300,
    (True, "rem16", "constant"): 56400,
    (True, "rem16", "replicate"): 56500,
    (True, "rem16", "circular"): 56600,
    (True, "rem16", "reflect"): 56700,
    (True, "c13", "constant"): 56800,
    (True, "c13", "replicate"): 56900,
    (True, "c13", "circular"): 57000,
    (True, "c13", "reflect"): 57100,
    (True, "fc128", "constant"): 57200,
    (True, "fc128", "replicate"): 57300,
    (True, "fc128", "circular"): 57400,
    (True, "fc128", "reflect"): 57500,
    (True, "cond4", "constant"): 57600,
    (True, "cond4", "replicate"): 57700,
    (True, "cond4", "circular"): 57800,
    (True, "cond4", "reflect"): 57900,
    (True, "persist", "constant"): 58000,
    (True, "persist", "replicate"): 58100,
    (True, "persist", "circular"): 58200,
    (True, "persist", "reflect"): 58300,
    (True, "ms14nc", "constant"): 58400,
    (True, "ms14nc", "replicate"): 58500,
    (True, "ms14nc", "circular"): 58600,
    (True, "ms14nc", "reflect"): 58700,
    (False, "p12", "constant"): 58800,
    (False, "p12", "replicate"): 58901,
    (False, "p12", "circular"): 59000,
    (False, "p12", "reflect"): 59100,
    (False, "p5", "constant"): 59200,
    (False, "p5", "replicate"): 59300,
    (False, "p5", "circular"): 59400,
    (False, "p5", "reflect"): 59500,
    (False, "p16", "constant"): 59600,
    (False, "p16", "replicate"): 59700,
    (False, "p16", "circular"): 59800,
    (False, "p16", "reflect"): 59900,
    (False, "p13", "constant"): 60000,
    (False, "p13", "replicate"): 60100,
    (False, "p13", "circular"): 60200,
    (False, "p13", "reflect"): 60300,
    (True, "p12", "constant"): 60400,
    (True, "p12", "replicate"): 60500,
    (True, "p12", "circular"): 60600,
    (True, "p12", "reflect"): 60700,
    (True, "p5", "constant"): 60800,
    (True, "p5", "replicate"): 60900,
    (True, "p5", "circular"): 61000,
    (True, "p5", "reflect"): 61100,
    (True, "p16", "constant"): 61200,
    (True, "p16", "replicate"): 61300,
    (True, "p16", "circular"): 61400,
    (True, "p16", "reflect"): 61500,
    (True, "p13", "constant"): 61600,
    (True, "p13", "replicate"): 61700,
    (True, "p13", "circular"): 61800,
    (True, "p13", "reflect"): 61900,
}


def geometry(two, row):
    """(C, fc, c_cond, B, H, W) of a row as the tests run it"""
    if row in PERSIST:
        return PERSIST[row][0]
    if two:
        C, fc, cc, H, W = ADDED_TWO[row] if row in ADDED_TWO else S2.CASES[row][:3] + S2.CASES[row][4:]
    else:
        C, fc, cc, H, W = ADDED_SINGLE[row] if row in ADDED_SINGLE else S1.CASES[row][:3] + S1.CASES[row][4:]
    return C, fc, cc, math.ceil(CELLS / (H * W)), H, W


def admits(two, row, pad):
    """reflect needs H, W >= 2 (the coarse level of the two-scale step too: H, W >= 4)"""
    _, _, _, _, H, W = geometry(two, row)
    return pad != "reflect" or min(H, W) >= (4 if two else 2)


def bf16_class(C, fc):
    """dispatch_dynca<DyncaFwdBf | DyncaFwdMsBf, kDynca12x96, kDynca16x128>; dispatch_persist's `small`"""
    return (12, 96) if C <= 12 and fc <= 96 else (16, 128) if C <= 16 and fc <= 128 else None


def bf16_form(H, W, addr=0):
    """launch_dynca_class with fp32 storage"""
    return "vec" if W % 4 == 0 and addr % 16 == 0 and (H * W) % 4 == 0 else "any"


ROWS = [(False, r) for r in SINGLE] + [(True, r) for r in TWO]
PERSIST_ROWS = [(two, r) for two in (False, True) for r in PERSIST]
ROW_PADS = [(two, r, p) for two, r in ROWS + PERSIST_ROWS for p in O.PAD_MODES if admits(two, r, p)]


def scales_of(two):
    return (0, 1) if two else (0,)


def make_inputs(two, row, pad, device="cpu", seed=None):
    """(prm, x, cond or None, us [T_MAX,B,1,H,W]) of a (row, pad): test_dynca_bf16_host.bf16_inputs at the table's seed; its
    uniforms are step 0's, the later steps' come from a generator of their own"""
    seed = SEEDS[two, row, pad] if seed is None else seed
    C, fc, cc, B, H, W = geometry(two, row)
    prm, x, cond, u = bf16_inputs(C, fc, cc, B, H, W, seed, device=device)
    more = torch.rand(T_MAX - 1, B, 1, H, W, generator=torch.Generator().manual_seed(seed + 1000003)).to(device)
    return prm, x, cond, torch.cat([u[None], more])


def host_figures(two, row, pad, seed=None, say=True):
    """the float64 restatement against the fp32 evaluation of the same contract at step 0 of a (row, pad):
    (cap-(b) fraction, E.max(), fraction of cells that fire); check_caps has passed when it returns"""
    prm, x, cond, us = make_inputs(two, row, pad, seed=seed)
    ref, E = contract_step(x, cond, us[0], prm, pad, scales=scales_of(two))
    got, _ = contract_step(x, cond, us[0], prm, pad, scales=scales_of(two), dtype=torch.float32)
    what = f"contract fp32 vs float64 {'two-scale ' if two else ''}{row} {geometry(two, row)} {pad}"
    with contextlib.nullcontext() if say else contextlib.redirect_stdout(io.StringIO()):
        _, frac = check_caps(got, ref, E, x, what)
    return frac, float(E.max()), float((us[0] + 0.5).floor().mean())


def qualifies(two, row, pad, seed):
    try:
        frac, emax, fired = host_figures(two, row, pad, seed, say=False)
    except AssertionError:
        return False
    return frac <= HALF_CAP and emax > 1e-4 and 0.25 < fired < 0.75


def search():
    """prints SEEDS: per (row, pad) the first qualifying seed from a base that depends on nothing but the row's place in the table"""
    for i, (two, row, pad) in enumerate(ROW_PADS):
        seed = 50000 + 100 * i
        while not qualifies(two, row, pad, seed):
            seed += 1
        print(f'    ({two}, "{row}", "{pad}"): {seed},', flush=True)


# ==================================================================================== 1. the rows and what they reach
def test_rows_are_the_table_rows_and_reach_every_class_in_both_forms():
    assert [r for r in SINGLE if r not in ADDED_SINGLE] == [c for c in S1.CASES if S1.CASES[c][0] <= 16 and S1.CASES[c][1] <= 128]
    assert [r for r in SINGLE if r not in ADDED_SINGLE] == ["one", "row", "c5", "h4", "w8", "band", "rem12", "rem16v", "c13", "fc128", "cond4"]
    assert [r for r in TWO if r not in ADDED_TWO] == list(S2.CASES)
    assert ADDED_SINGLE == {"c14nc": (14, 100, 0, 3, 5)} and ADDED_TWO == {"ms14nc": (14, 100, 0, 6, 10)}
    every = {(cls, cond, form) for cls in ((12, 96), (16, 128)) for cond in (True, False) for form in ("vec", "any")}
    for two, table in ((False, SINGLE), (True, TWO)):
        seen = set()
        for row, (cls, has_cond, form) in table.items():
            C, fc, cc, B, H, W = geometry(two, row)
            assert B == math.ceil(CELLS / (H * W)) and B * H * W >= CELLS and (B - 1) * H * W < CELLS, row
            assert bf16_class(C, fc) == cls and (cc > 0) == has_cond and bf16_form(H, W) == form, (two, row)
            assert not two or (H % 2 == 0 and W % 2 == 0), row
            assert form == "any" or (B * C * H * W) % 4 == 0, row      # every slot of a kept history is 16-byte aligned where the first is
            seen.add((cls, has_cond, form))
        assert seen == every and len(seen) == 8, (two, every - seen)
    assert max(B * H * W for _, _, _, B, H, W in (geometry(two, r) for two, r in ROWS)) == 1920       # cond4: two planes of 960 cells
    assert bf16_form(4, 12, addr=4) == "any"                           # a view one float into its buffer at W % 4 == 0


def test_persistent_rows_reach_all_eight_instantiations():
    assert [PERSIST[r][0] for r in PERSIST] == [(12, 96, 3, 1, 16, 32), (5, 24, 0, 2, 16, 16), (16, 128, 4, 1, 32, 16), (13, 104, 0, 1, 16, 32)]
    seen = set()
    for two, row in PERSIST_ROWS:
        (C, fc, cc, B, H, W), cls, has_cond = PERSIST[row]
        assert geometry(two, row) == (C, fc, cc, B, H, W)
        assert bf16_class(C, fc) == cls and (cc > 0) == has_cond and H % 16 == 0 and W % 16 == 0, row
        seen.add((two, cls, has_cond))
    assert len(seen) == 8
    assert any(PERSIST[r][0][3] > 1 for r in PERSIST)                  # a batch above one


def test_every_row_and_pad_has_a_seed():
    assert set(SEEDS) == set(ROW_PADS)
    assert len(set(SEEDS.values())) == len(SEEDS)
    for two, row in ROWS + PERSIST_ROWS:
        pads = [p for p in O.PAD_MODES if admits(two, row, p)]
        _, _, _, _, H, W = geometry(two, row)
        assert pads == [p for p in O.PAD_MODES if p != "reflect" or min(H, W) >= (4 if two else 2)] and len(pads) >= 3


# ==================================================================================== 2. the comparator is fair on every (row, pad)
@pytest.mark.parametrize("two,row", ROWS + PERSIST_ROWS, ids=lambda v: v if isinstance(v, str) else ("two_scale" if v else "single"))
def test_reference_alone_stays_inside_half_of_cap_b(two, row):
    """float64 restatement against the fp32 evaluation of the same contract: inside cap (a), at most HALF of cap (b), and the row
    is not vacuous"""
    for pad in O.PAD_MODES:
        if not admits(two, row, pad):
            continue
        frac, emax, fired = host_figures(two, row, pad)
        print(f"   cap-(b) fraction {100 * frac:.3f} % (half cap {100 * HALF_CAP:g} %), E.max {emax:.3g}, cells that fire {100 * fired:.1f} %")
        assert frac <= HALF_CAP, (row, pad, frac)
        assert emax > 1e-4 and 0.25 < fired < 0.75, (row, pad, emax, fired)


# ==================================================================================== 3. the caps catch what they are for
def _zeroed(prm, name, index):
    """a copy of prm with prm[name][index] = 0"""
    bad = dict(prm)
    bad[name] = prm[name].clone()
    bad[name][index] = 0
    return bad


#           row      pad          tensor        index                          what a kernel with this slip would have lost
WEIGHT_CONTROLS = [("cond4", "replicate", "w1.weight", (slice(None), 4 * 16 + 3), "the last of four conditioning lanes (gg < CC)"),
                   ("row", "circular", "w1.weight", (slice(None), 4 * 8), "its only conditioning lane"),
                   ("c5", "replicate", "w2.weight", (slice(None), slice(16, None)), "the partial hidden tile of fc = 24 (k < fc)"),
                   ("c14nc", "constant", "w2.weight", (slice(None), slice(96, None)), "the last four hidden units of fc = 100"),
                   ("c13", "reflect", "w2.weight", (slice(None), slice(96, None)), "the last eight hidden units of fc = 104"),
                   ("c5", "circular", "w1.weight", (slice(None), 4), "channel 4's identity column: the partial channel group of C = 5 (ch < C)"),
                   ("c13", "replicate", "w1.weight", (slice(None), 12), "channel 12's identity column: the fourth channel group of C = 13")]


@pytest.mark.parametrize("row,pad,name,index,what", WEIGHT_CONTROLS, ids=[f"{c[0]}-{c[2]}-{i}" for i, c in enumerate(WEIGHT_CONTROLS)])
def test_caps_catch_a_lost_weight_edge(row, pad, name, index, what):
    prm, x, cond, us = make_inputs(False, row, pad)
    ref, E = contract_step(x, cond, us[0], prm, pad)
    good, _ = contract_step(x, cond, us[0], prm, pad, dtype=torch.float32)
    check_caps(good, ref, E, x, f"control {row} {pad} unmodified")                         # the unmodified evaluation passes
    bad = _zeroed(prm, name, index)
    assert int((bad[name] != prm[name]).sum()) > 0
    got, _ = contract_step(x, cond, us[0], bad, pad, dtype=torch.float32)
    with pytest.raises(AssertionError):
        check_caps(got, ref, E, x, f"control {row} {pad} without {what}")


#               two    row       the run's pad   the wrong pad
PAD_CONTROLS = [(False, "cond4", "replicate", "constant"),
                (False, "rem16v", "reflect", "circular"),
                (True, "rem16", "circular", "replicate")]


@pytest.mark.parametrize("two,row,pad,wrong", PAD_CONTROLS, ids=[f"{c[1]}-{c[3]}-for-{c[2]}" for c in PAD_CONTROLS])
def test_caps_catch_a_wrong_pad_mode(two, row, pad, wrong):
    prm, x, cond, us = make_inputs(two, row, pad)
    ref, E = contract_step(x, cond, us[0], prm, pad, scales=scales_of(two))
    good, _ = contract_step(x, cond, us[0], prm, pad, scales=scales_of(two), dtype=torch.float32)
    check_caps(good, ref, E, x, f"control {row} {pad} unmodified")
    got, _ = contract_step(x, cond, us[0], prm, wrong, scales=scales_of(two), dtype=torch.float32)
    with pytest.raises(AssertionError):
        check_caps(got, ref, E, x, f"control {row}: {wrong} for {pad}")


if __name__ == "__main__":
    torch.set_num_threads(1)
    search()
