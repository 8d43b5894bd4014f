"""The ConditionedNCA step and its backward against float64 at the smallest shape of every class: the sibling of
test_gpu_dynca_ref.py for the kernels bench.py's `value` runs on (csrc/nca_cond_generic.hip, nca_cond_pc.hip, nca_cond_bwd.hip,
nca_cond_bwd_fm.hip, nca_cond_persist.hip).

Method, that of test_gpu_cond_replay.py: the kernels record their own history (keep_history=True) and the float64 oracle is
restarted from the recorded input of every step (nca_oracle.cond_replay_forward / cond_replay_vjp), so every mask is demanded
exactly and nothing is excluded.  Bounds, the project's own: util.REPLAY_TOL (1e-5) for one replayed step, util.REL_TOL (1e-4) for
every stored state of the free-running float64 trajectory, GTOL (2e-4 of the largest reference entry) for all eight gradients.

Seeds.  Every small row's input seed is a literal found on the CPU against float64 alone (search() below; run this file directly
to regenerate the table).  A seed qualifies when, along the float64 trajectory, no gradient-carrying ReLU gate lies within SAFETY *
GATE_K (SAFETY = 4) of zero and no cell has its 3 x 3-pooled alpha, before or after an update, within NEAR_EPS of float32(0.1).  On
the GPU every float64 comparison asserts zero gates within GATE_K on the recorded history.  Two kinds of rows cannot have such a
seed and say so where they are defined: the form-selection rows (LARGE: 1e3 .. 2e5 cells, where a trajectory holds tens of such
gates whatever the seed) and the bf16 rows (the recorded bf16 history differs from any CPU emulation by final-rounding flips, so its
gates are only known on the GPU).  There the cotangent is ZEROED where it could reach such a gate -- within Chebyshev distance
T - 1 - t of a gate of step t, found on the recorded history at SAFETY * GATE_K -- so the gate's cotangent is an exact zero on both
sides and still every element of every gradient is compared.

Every test prints its measured errors next to the bounds (-s)."""
import os
import sys

if __name__ == "__main__":      # the seed search runs without the suite's conftest: the same import paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "video-stylization-with-nca_amd")]

import pytest
import torch
import torch.nn.functional as F

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from test_gpu_configs import rand_cond_prm
from test_gpu_cond_replay import Draws, _bf16_case, _cost, _grad_errs, _lever, _replay   # noqa: F401  (_cost: time per test)
from test_gpu_fullsize_ref import COND_NAMES, GTOL, _cond_w, _f64, _rel, _rel2, _rmax, _say
from util import GATE_K, REL_TOL, REPLAY_TOL, near_threshold

pytestmark = pytest.mark.gpu
DEV = "cuda"
TN = 3
SAFETY = 4                  # the seed search (and the zeroed cotangents) keep gates SAFETY * GATE_K away: the state a kernel stores
#                             differs from the float64 trajectory by ~1e-6 relative, which moves a gate's margin by about GATE_K
NEAR_EPS = 1e-4             # near_threshold's default
PHILOX_KEY = 0x5EED0003     # the key of every in-kernel Philox row (steps 0 .. T - 1)
ONE_WG = 1 << 8             # ncahip_debug_force_generic bits 8-15: one workgroup walks every tile in rounds, the carry crosses tiles

# What each row reaches, read off the launchers.  CUs = 256 (MI355X) in the comments; the tests take the count from the device.
#   fwd   nca_launch_cond_step_fwd: W % 4 == 0 and C <= 20 -> nca_launch_cond_step_fwd_pc = launch_cond_pc<CP, EXACT, StF32, false, FC, CARRY>,
#         EXACT iff C == CP and hidden == 64; default FC + CARRY at CP <= 16, FC without CARRY at CP = 20 and under force 64, dense under
#         force 32; wave tile 4 x 16, super-tile 16 x 16, nwg = min(nst, CUs), nst = B ceil(W/16) ceil(H/16).  Force 2 (C <= 16): the wave
#         kernel.  Force 1, W % 4 != 0 and every C > 20: launch_cond<12|16|20|24|32> (csrc/nca_cond_generic.hip, 8 x 32 tiles), VEC iff W % 4 == 0.
#   A     nca_launch_cond_step_bwd: C <= 16 -> launch_bwd<12|16, StF32>: front + matrix (launch_fm<CP, StF32, false>) iff 2 nst <= CUs, else
#         one launch; C > 16 -> launch_fm<20|24|32> always.  The front kernel's last template flag is C == CP; msplit iff 2 nst <= CUs.
#   B     cond_step_bwd_stencil_kernel<float, srows>, srows from stencil_srows: 4 on every small grid.
#        id          B   C  hidden  H   W  goal alive rate  masks
CASES = {"g1x4":    (3, 12, 64,     1,  4,  8,  3, 0.5, "uniform"),   # one 4-cell group, B = 3.  fwd pc<12,EXACT>; A fm<12> front<C==CP> msplit; B <float,4>
         "g2x4":    (1, 9,  40,     2,  4,  5,  3, 0.5, "bits"),      # B = 1, padded channels and hidden units.  fwd pc<12,!EXACT>; A fm<12> front<C!=CP> msplit; B 4
         "g3x8":    (2, 16, 64,     3,  8,  12, 3, 0.5, "philox"),    # H below the alive halo of 3.  fwd pc<16,EXACT>; A fm<16> front<C==CP> msplit; B 4
         "g4x16":   (2, 13, 48,     4,  16, 9,  3, 0.5, "uniform"),   # exactly one wave tile.  fwd pc<16,!EXACT>; A fm<16> front<C!=CP> msplit; B 4
         "g5x20":   (1, 20, 64,     5,  20, 16, 3, 0.5, "bits"),      # one row and one column group past a wave tile.  fwd pc<20,EXACT> (no carry); A fm<20,StF32> front<C==CP> msplit, 4 waves; B 4
         "g16x16":  (1, 18, 48,     16, 16, 14, 3, 0.5, "philox"),    # exactly one super-tile.  fwd pc<20,!EXACT>; A fm<20> front<C!=CP> msplit; B 4
         "g17x20":  (1, 16, 64,     17, 20, 12, 3, 0.5, "uniform"),   # remainder super-tiles in both directions (nst = 4).  fwd pc<16,EXACT>; A fm<16> msplit; B 4
         "g18x68":  (1, 12, 64,     18, 68, 8,  3, 0.5, "bits"),      # nst = 10, a third 8 x 32 tile row and column for the generic kernel.  fwd pc<12,EXACT>; A fm<12> msplit; B 4.  NEAR_EPS 1e-5, see NEAR
         "c24":     (1, 24, 64,     5,  20, 20, 3, 0.5, "uniform"),   # smallest CP = 24.  fwd launch_cond<24> VEC (every family: C > 20); A launch_fm<24,StF32,false> front<C==CP>; B 4
         "c17":     (1, 17, 16,     17, 20, 13, 3, 0.5, "bits"),      # fwd pc<20,!EXACT>, force 1 launch_cond<20> VEC; A launch_fm<20> front<C!=CP> (C = 17 is CP = 20 in both launchers, not 24: fm_cp); B 4
         "c21":     (2, 21, 16,     4,  16, 17, 3, 0.5, "philox"),    # the smallest C that pads to 24.  fwd launch_cond<24> VEC; A launch_fm<24> front<C!=CP>; B 4
         "c32":     (1, 32, 64,     4,  16, 28, 3, 0.5, "philox"),    # fwd launch_cond<32> VEC; A launch_fm<32,StF32,false,NCA_FM_NT32> front<C==CP>; B 4
         "c25":     (1, 25, 28,     17, 20, 21, 3, 0.5, "uniform"),   # fwd launch_cond<32> VEC; A launch_fm<32,..,NCA_FM_NT32> front<C!=CP>, padded hidden units; B 4
         "goal0":   (3, 16, 64,     5,  20, 0,  3, 0.5, "philox"),    # goal_ch = 0 (goal = NULL), B = 3.  fwd pc<16,EXACT>; A fm<16> msplit; B 4
         "goalC":   (1, 12, 64,     17, 20, 12, 3, 0.5, "bits"),      # goal_ch = C.  fwd pc<12,EXACT>; A fm<12> msplit; B 4
         "nolife":  (2, 13, 48,     5,  20, 9, -1, 0.5, "uniform"),   # alive_ch = -1: halo 1, no mask read.  fwd pc<16,!EXACT>; A fm<16> front<C!=CP>; B 4
         "nolife20": (1, 20, 64,    17, 20, 16, -1, 0.5, "philox"),   # the same at CP = 20.  fwd pc<20,EXACT>; A fm<20>; B 4
         "rate0":   (2, 12, 64,     5,  20, 8,  3, 0.0, "uniform"),   # no cell fires: empty firing-cell lists, zero weight gradients.  fwd pc<12,EXACT>; A fm<12>; B 4
         "rate025": (3, 20, 64,     5,  20, 16, 3, 0.25, "bits"),     # sparse lists, B = 3.  fwd pc<20,EXACT>; A fm<20>; B 4
         "rate1":   (2, 16, 64,     4,  16, 12, 3, 1.0, "philox"),    # every cell fires: full groups only.  fwd pc<16,EXACT>; A fm<16>; B 4
         "clamp":   (1, 16, 64,     5,  20, 12, 3, 0.5, "uniform"),   # inputs up to +-9.8: firing cells land on the clamp at +-10 (asserted).  fwd pc<16,EXACT>; A fm<16>; B 4
         # W % 4 != 0, one row per CP, forward only: launch_cond<CP> scalar; ncahip_cond_grow_bwd_f32 refuses the width
         "w10c12":  (2, 12, 64,     5,  10, 8,  3, 0.5, "uniform"),
         "w10c16":  (2, 13, 48,     5,  10, 9,  3, 0.5, "philox"),
         "w10c20":  (2, 20, 64,     5,  10, 16, 3, 0.5, "uniform"),
         "w10c24":  (2, 24, 64,     5,  10, 20, 3, 0.5, "philox"),
         "w10c32":  (2, 25, 28,     5,  10, 21, 3, 0.5, "uniform"),
         # form selection (LARGE): no seed has zero gates here, the cotangent is zeroed around them; no free-running comparison
         "b129":    (129, 16, 64,   2,  4,  12, 3, 0.5, "philox"),    # 128 < nst = 129 <= CUs: the default form of kernel A is ONE launch, launch_bwd<16,StF32> (asserted); B 4
         "walk":    (33, 16, 64,    17, 52, 12, 3, 0.5, "bits"),      # nst = 33 * 2 * 4 = 264 > CUs: a workgroup walks a second super-tile, every slab row is reduced; one launch by default; B 4
         "sr8":     (17, 16, 64,    68, 68, 12, 3, 0.5, "philox"),    # stencil_srows = 8 (asserted): 272 planes of 17 x 17 four-cell groups: two blocks per plane at 4 rows, one at 8.  T = 2
         "sr16":    (17, 16, 64,    64, 200, 12, 3, 0.5, "bits")}     # stencil_srows = 16 (asserted): 50 groups per row: one block per plane only at 16 rows.  T = 2
LARGE = ("b129", "walk", "sr8", "sr16")
T_OF = {"sr8": 2, "sr16": 2}
SROWS = {"sr8": 8, "sr16": 16}
# 18 x 68 = 1224 cells: a trajectory holds ~20 cells within 1e-4 of the threshold whatever the seed (the density of the pooled alpha of
# x0[:, alive] *= 0.12 at 0.1 is ~17 per unit: 3.5e-3 per cell and state).  1e-5 is still ten times the ~1e-6 by which a stored state
# differs from the float64 trajectory.
NEAR = {"g18x68": 1e-5}
W10 = tuple(c for c in CASES if CASES[c][4] % 4)
SMALL = tuple(c for c in CASES if c not in LARGE and c not in W10)
PRM_SEED = {k: 900 + i for i, k in enumerate(CASES)}

# input seeds (x0, goal, cotangent: make_inputs; uniforms: seed + 1) found by search() on the CPU in float64; LARGE rows: any seed
SEEDS = {
    "g1x4": 1000, "g2x4": 2000, "g3x8": 3000, "g4x16": 4000, "g5x20": 5002, "g16x16": 6001, "g17x20": 7001, "g18x68": 8001,
    "c24": 9000, "c17": 10000, "c21": 11000, "c32": 12000, "c25": 13001, "goal0": 14004, "goalC": 15005, "nolife": 16000,
    "nolife20": 17002, "rate0": 18000, "rate025": 19001, "rate1": 20000, "clamp": 21200, "w10c12": 22000, "w10c16": 23001,
    "w10c20": 24001, "w10c24": 25000, "w10c32": 26000, "b129": 27000, "walk": 28000, "sr8": 29000, "sr16": 30000,
}
SEED_BASE = {k: 1000 * (i + 1) for i, k in enumerate(CASES)}

# bf16 history: CP 12, 16, 20, EXACT and not, each at 4 x 16 (one wave tile), 5 x 20 and 17 x 20 (remainders); goal C - 4; B = 6, 4, 2 so that
# every row has some hundred cells (the bf16 bounds are relative L2 over gate flips: they need a population)
BF16_CH = {"c12": (12, 64), "c9": (9, 40), "c16": (16, 64), "c13": (13, 48), "c20": (20, 64), "c18": (18, 48)}
BF16_SHAPES = {"4x16": (4, 16), "5x20": (5, 20), "17x20": (17, 20)}
BF16_B = {"4x16": 6, "5x20": 4, "17x20": 2}
BF16_CASES = [(c, s) for c in BF16_CH for s in BF16_SHAPES]


# ================================================================================================ inputs, float64 trajectory, seed search (CPU)
def make_inputs(case, seed):
    """(prm, x0, goal or None, cot) of a row on the CPU, all from literal seeds; alpha on both sides of the threshold"""
    B, C, hid, H, W, gch, alive, rate, mode = CASES[case]
    prm = rand_cond_prm(C, seed=PRM_SEED[case], hidden=hid, out_scale=1.0)
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=gen)
    if alive >= 0:
        x0[:, alive] *= 0.12
    if case == "clamp":
        alpha = x0[:, alive].clone()
        x0 = (x0 - 0.5) * 19.6
        x0[:, alive] = alpha
    goal = torch.randn(B, gch, H, W, generator=gen) * 0.5 if gch else None
    cot = torch.randn(B, C, H, W, generator=gen)
    return prm, x0, goal, cot


def cpu_draws(case, seed):
    """what Draws(mode, gen_seed=seed + 1, seed=PHILOX_KEY).u(k) holds, without a device: uniforms, 1 - mask, or the Philox draws"""
    B, C, hid, H, W, gch, alive, rate, mode = CASES[case]
    Tn = T_OF.get(case, TN)
    if mode == "philox":
        return [torch.from_numpy(O.philox_uniform(PHILOX_KEY, k, B, H, W)) for k in range(Tn)]
    us = torch.rand(Tn, B, 1, H, W, generator=torch.Generator().manual_seed(seed + 1))
    return [u if mode == "uniform" else 1.0 - (u.clamp(0.0, 1.0) < rate).float() for u in us]


def f64_trajectory(x0, gpad, us, p64, alive, rate):
    """the float64 O.cond_step trajectory from x0: per step (input, pre mask, pending x + r * out, life mask)"""
    x, steps = x0.double(), []
    gz = torch.zeros_like(x) if gpad is None else gpad
    with torch.no_grad():
        for u in us:
            d = O.cond_step(x, gz, u.to(x.device), p64, alive, 0.1, rate, use_living_channel=alive >= 0, return_all=True)
            steps.append((x, d["pre"], d["x1"], d["life"]))
            x = d["x2"]
    return steps, x


def qualifies(case, seed, safety=SAFETY):
    """the seed criterion, float64 on the CPU only: (ok, gates within safety * GATE_K, near-threshold cells, clamped elements)"""
    B, C, hid, H, W, gch, alive, rate, mode = CASES[case]
    eps = NEAR.get(case, NEAR_EPS)
    prm, x0, goal, _ = make_inputs(case, seed)
    if alive >= 0 and bool(near_threshold(x0, alive, eps=eps).any()):
        return False, -1, -1, 0
    p64 = {k: v.double() for k, v in prm.items()}
    gpad = None if goal is None else O.cond_pad_goal(goal.double(), C)
    us = cpu_draws(case, seed)
    steps, _ = f64_trajectory(x0, gpad, us, p64, alive, rate)
    near = 0 if alive < 0 else sum(int(near_threshold(s, alive, eps=eps).sum()) for x, _, x1, _ in steps for s in (x, x1))
    gz = torch.zeros_like(x0.double()) if gpad is None else gpad
    gates = int(O.cond_gate_influence(x0.double(), gz, us, p64, alive, safety * GATE_K, 0.1, rate, alive >= 0)[1].sum())
    live = [(x1 * life).abs() for _, _, x1, life in steps]
    clamped = sum(int((v > 10.0).sum()) for v in live)
    at_edge = sum(int(((v - 10.0).abs() < 1e-4).sum()) for v in live)
    ok = near == 0 and at_edge == 0 and (gates == 0 or case in W10) and (case != "clamp" or clamped > 0)
    return ok, gates, near, clamped


def search(cases=None, tries=200000):
    """first qualifying seed at or after SEED_BASE of every row that needs one: prints the SEEDS table"""
    for case in cases or (SMALL + W10):
        for seed in range(SEED_BASE[case], SEED_BASE[case] + tries):
            ok, gates, near, clamped = qualifies(case, seed)
            if ok:
                print(f'    "{case}": {seed},' + (f"    # {clamped} clamped elements" if case == "clamp" else ""), flush=True)
                break
        else:
            print(f"    # {case}: no seed among {tries}", flush=True)


# ================================================================================================ Python restatements of the form selection
def n_super_tiles(B, H, W):
    return B * ((W + 15) // 16) * ((H + 15) // 16)


def kernel_a_form(B, C, H, W, cus, force=0, bfm=False):
    """(front + matrix?, msplit?) of kernel A: narrow_is_fm (csrc/nca_cond_bwd.hip) and launch_fm's msplit (csrc/nca_cond_bwd_fm.hip);
    nslab = the CU count (nca_cond_bwd_nslab); force bit 3 = the other form (C <= 16), bit 4 = no split; bfm = products on bf16 MFMA"""
    nst = n_super_tiles(B, H, W)
    default_fm = bfm or 2 * nst <= cus
    fm = True if C > 16 else (default_fm != bool(force & 8))
    return fm, bool(fm and not (force & 16) and 2 * nst <= cus)


def stencil_srows(B, C, H, W, cus):
    """stencil_srows of csrc/nca_cond_bwd.hip: rounds of resident waves x (rows + 2 halo rows), smallest wins, ties to the taller"""
    slots, best, best_cost = cus * 8, 16, None
    for sr in (16, 8, 4):
        per_plane = ((H + sr - 1) // sr) * (W // 4)
        waves = B * C * ((per_plane + 255) // 256) * 4
        cost = ((waves + slots - 1) // slots) * (sr + 2)
        if best_cost is None or cost < best_cost:
            best, best_cost = sr, cost
    return best


def cu_count():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ================================================================================================ the kernels and their float64 reference
@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=False) as o:
        yield o


def _forced(ops, force, fn, *a, **kw):
    ops.force_generic(force)
    try:
        r = fn(*a, **kw)
        ops.check_errors()
        return r
    finally:
        ops.force_generic(0)


def _in(states, pre, k, alive):
    """the recorded input of step k in the history's dtype"""
    return states[0] if k == 0 else O.cond_resolve(states[k], pre[k], alive)


def quiet_cotangent(cot, states, pre, gpad, dr, p64, alive, rate, k=SAFETY * GATE_K):
    """cot with zeros wherever it could reach a gradient-carrying gate within k of zero: a gate of step t at cell c sees dL/d in_{t+1}(c),
    which g_final reaches from Chebyshev distance T - 1 - t at most.  Returns (cot, gates found, fraction of cells zeroed)."""
    Tn = states.shape[0] - 1
    keep = torch.ones_like(cot[:, :1], dtype=torch.bool)
    n = 0
    for t in range(Tn):
        x_in = states[0].double() if t == 0 else O.cond_resolve(states[t].double(), pre[t], alive)
        cells, cnt = O.cond_replay_gates(x_in, states[t + 1], pre[t + 1], gpad, dr.u(t), p64, alive, k, fire_rate=rate)
        r = Tn - 1 - t
        keep &= ~(F.max_pool2d(cells.float(), 2 * r + 1, 1, r) > 0)
        n += int(cnt.sum())
    return cot * keep, n, 1.0 - float(keep.float().mean())


_RUNS = {}


def run(ops, case):
    """inputs, the default kernels' recorded history and the float64 replay VJP of a row: computed once, shared, left unchanged"""
    if case in _RUNS:
        return _RUNS[case]
    B, C, hid, H, W, gch, alive, rate, mode = CASES[case]
    Tn = T_OF.get(case, TN)
    prm, x0, goal, cot = make_inputs(case, SEEDS[case])
    x0, cot, goal = x0.to(DEV), cot.to(DEV), None if goal is None else goal.to(DEV)
    dr = Draws(ops, mode, B, H, W, Tn, rate, seed=PHILOX_KEY, gen_seed=SEEDS[case] + 1)
    r = dict(case=case, prm=prm, p64=_f64(prm), x0=x0, goal=goal, dr=dr, w=_cond_w(ops, prm, x0), Tn=Tn, alive=alive, rate=rate, C=C,
             gch=gch, gpad=None if goal is None else O.cond_pad_goal(goal.double(), C))
    out, states, pre = grow(ops, r, 0, True)
    r.update(out=out.clone(), states=states, pre=pre)
    if W % 4 == 0:
        if case in LARGE:
            cot, r["gates_quiet"], r["zeroed"] = quiet_cotangent(cot, states, pre, r["gpad"], dr, r["p64"], alive, rate)
        r["gates"] = int(O.cond_replay_gate_region(states, pre, r["gpad"], dr, r["p64"], alive, GATE_K, fire_rate=rate)[1].sum())
        r["steps"] = {}
        r["ref"] = O.cond_replay_vjp(states, pre, r["gpad"], dr, r["p64"], cot, alive, fire_rate=rate,
                                     on_step=lambda k, x_in, g_next, res: r["steps"].__setitem__(k, (g_next, res)))
    r["cot"] = cot
    _RUNS[case] = r
    return r


def grow(ops, r, force, hist):
    res = _forced(ops, force, ops.cond_grow, r["x0"], r["Tn"], r["goal"], r["dr"].arg, r["w"], r["alive"], fire_rate=r["rate"],
                  seed=r["dr"].seed, keep_history=hist)
    torch.cuda.synchronize()
    return res


def backward(ops, r, force, states=None, goal=None, cot=None):
    states = r["states"] if states is None else states
    return _forced(ops, force, ops.cond_grow_backward, states, r["pre"], r["goal"] if goal is None else goal, r["dr"].arg, r["w"],
                   r["cot"] if cot is None else cot, r["Tn"], r["alive"], fire_rate=r["rate"], seed=r["dr"].seed)


def _pick(case):
    return f"seed {SEEDS[case]} of row {case} puts gates within {GATE_K} of zero on the recorded history: pick another (search())"


def families(case):
    """(name, ncahip_debug_force_generic value) of every forward family that takes the row"""
    B, C, hid, H, W = CASES[case][:5]
    if W % 4 or C > 20:
        return [("default = generic", 0)]
    fam = [("default", 0), ("no carry", 64), ("dense", 32), ("generic VEC", 1), ("one workgroup", ONE_WG), ("one workgroup, no carry", ONE_WG | 64)]
    return fam + ([("wave", 2)] if C <= 16 else [])


# ================================================================================================ forward
@pytest.mark.parametrize("case", list(CASES))
def test_forward_replayed(ops, case):
    """every forward family: pre masks exact, non-firing cells kept by value, firing cells within REPLAY_TOL of float64 from the same
    input, x_final == cond_resolve(slot T), the keep_history=False (ring 2) call equal to it.  Nothing excluded."""
    r = run(ops, case)
    for name, force in families(case):
        out, states, pre = (r["out"], r["states"], r["pre"]) if force == 0 else grow(ops, r, force, True)
        out = out.clone()
        ring2, _, _ = grow(ops, r, force, False)
        worst, near, _ = _replay(states, pre, out, r["gpad"], r["dr"], r["p64"], r["alive"], r["rate"])
        same = torch.equal(ring2, out)
        _say(f"{case} {CASES[case]} fwd [{name}]", pre_mismatch=worst["pre"], nonfiring_changed=worst["keep"], firing_worst=worst["fire"],
             bound=REPLAY_TOL, final_mismatch=worst["final"], ring2_equal=same, near_threshold_cells_checked=near)
        assert worst["pre"] == 0 and worst["keep"] == 0 and worst["final"] == 0, (name, worst)
        assert worst["fire"] <= REPLAY_TOL, (name, worst)
        assert same, name
    if case == "clamp":
        n = sum(int((O.cond_resolve(r["states"][k + 1], r["pre"][k + 1], 3, lo=-1e30, hi=1e30).abs() > 10.0).sum()) for k in range(r["Tn"]))
        _say("clamp row", elements_beyond_the_clamp=n)
        assert n > 0, "the clamp row clamps nothing"


@pytest.mark.parametrize("case", SMALL + W10)
def test_forward_free_running(ops, case):
    """every stored state within REL_TOL of the float64 O.cond_step trajectory from x0, masks equal (the seed keeps the pooled alpha
    NEAR_EPS away from the threshold along that trajectory)"""
    r = run(ops, case)
    steps, xT = f64_trajectory(r["x0"], r["gpad"], [r["dr"].u(k) for k in range(r["Tn"])], r["p64"], r["alive"], r["rate"])
    worst, masks = 0.0, 0
    for k, (_, pre, x1, _) in enumerate(steps):
        worst = max(worst, _rel(r["states"][k + 1], x1))
        if r["alive"] >= 0:
            masks += int((r["pre"][k + 1].bool() != pre[:, 0]).sum())
    final = _rel(r["out"], xT)
    _say(f"{case} free-running", states_worst=worst, final=final, bound=REL_TOL, mask_mismatch=masks)
    assert masks == 0 and worst < REL_TOL and final < REL_TOL


@pytest.mark.parametrize("case", W10)
def test_unaligned_width_backward_refused(ops, case):
    from ncahip._capi import NcaHipError
    r = run(ops, case)
    with pytest.raises(NcaHipError):
        backward(ops, r, 0)
    ops.check_errors()


# ================================================================================================ backward
@pytest.mark.parametrize("case", SMALL + LARGE)
def test_backward_vs_float64(ops, case):
    """cond_grow_backward over the recorded T steps in the three forms of kernel A (force 0, 16, 8 | 16) and the T = 1 backward of every
    single step, all eight gradients against cond_replay_vjp at GTOL, nothing excluded (zero gates within GATE_K asserted; LARGE rows:
    the cotangent zeroed around them).  Forms that do not split super-tiles agree bit for bit, the split form within 2e-6
    (test_cond_backward_kernel_forms_agree's rule)."""
    r = run(ops, case)
    B, C, hid, H, W, gch, alive, rate, mode = CASES[case]
    if case in LARGE:
        _say(f"{case} cotangent", gates_within_4_GATE_K=r["gates_quiet"], cells_zeroed_fraction=r["zeroed"])
        assert int((r["cot"] != 0).sum()) > 0.5 * r["cot"].numel()
    else:
        assert r["gates"] == 0, _pick(case)
    cus, got = cu_count(), {}
    for force in (0, 16, 8 | 16):
        g = backward(ops, r, force)
        e = _grad_errs(g, *r["ref"], C, gch)
        fm, split = kernel_a_form(B, C, H, W, cus, force)
        _say(f"{case} {CASES[case]} bwd T={r['Tn']} [force {force}: {'front + matrix' if fm else 'one launch'}{', split' if split else ''}]",
             **e, bound=GTOL)
        for k, v in e.items():
            assert v < GTOL, (force, k, e)
        got[force] = (g, split)
    base, base_split = got[8 | 16]
    assert not base_split
    for force in (0, 16):
        g, split = got[force]
        for k in base:
            if base[k] is None:
                continue
            if split:
                d = float((g[k] - base[k]).abs().max()) / max(1e-12, float(base[k].abs().max()))
                assert d <= 2e-6, (force, k, d)
            else:
                assert torch.equal(g[k], base[k]), (force, k)
    worst = 0.0
    for k in range(r["Tn"]):                # one step alone, from the float64 adjoint of its output rounded to fp32
        us, seed, step0 = r["dr"].at(k)
        st = torch.stack([_in(r["states"], r["pre"], k, alive), r["states"][k + 1]])
        g_next, ref = r["steps"][k]
        g = ops.cond_grow_backward(st, torch.stack([r["pre"][k + 1]] * 2), r["goal"], us, r["w"], g_next.float(), 1, alive, fire_rate=rate,
                                   seed=seed, step0=step0)
        ops.check_errors()
        e = _grad_errs(g, *ref, C, gch)
        worst = max(worst, max(e.values()))
        assert max(e.values()) < GTOL, (k, e)
    _say(f"{case} bwd per step (T = 1)", worst=worst, bound=GTOL)


def test_form_selection(ops):
    """the rows built for a form of kernel A or a strip height of kernel B land there on this device (restatements above)"""
    cus = cu_count()
    for case in SMALL:
        B, C, hid, H, W = CASES[case][:5]
        assert stencil_srows(B, C, H, W, cus) == 4, case
        assert kernel_a_form(B, C, H, W, cus) == (True, True), case                     # front + matrix, split
        assert kernel_a_form(B, C, H, W, cus, 16) == (True, False), case
        assert kernel_a_form(B, C, H, W, cus, 8 | 16) == (C > 16, False), case          # one launch where it exists
    B, C, hid, H, W = CASES["b129"][:5]
    nst = n_super_tiles(B, H, W)
    _say("form selection", cus=cus, b129_nst=nst, walk_nst=n_super_tiles(*[CASES["walk"][i] for i in (0, 3, 4)]),
         srows={c: stencil_srows(*[CASES[c][i] for i in (0, 1, 3, 4)], cus) for c in LARGE})
    assert cus // 2 < nst <= cus and kernel_a_form(B, C, H, W, cus) == (False, False)    # one launch by default, a slab per super-tile
    assert kernel_a_form(B, C, H, W, cus, 8) == (True, False)
    B, C, hid, H, W = CASES["walk"][:5]
    assert n_super_tiles(B, H, W) > cus and kernel_a_form(B, C, H, W, cus) == (False, False)
    for case in LARGE:
        B, C, hid, H, W = CASES[case][:5]
        assert stencil_srows(B, C, H, W, cus) == SROWS.get(case, 4), case


# ================================================================================================ persistent grow, called directly
@pytest.mark.parametrize("C,shape", [(12, (1, 16, 16)), (16, (1, 16, 16)), (20, (1, 16, 16)), (9, (2, 32, 48)), (13, (2, 32, 48)),
                                     (18, (2, 32, 48))])
def test_persistent_grow_direct(ops, C, shape):
    """ncahip_cond_grow_fwd_persist_f32 = launch_cond_persist<12|16|20> called through the C ABI (return code 0: no fallback can hide),
    at one tile and at 2 x 2 x 3 tiles, against the float64 replay and bit for bit against the per-step kernels.  The entry point
    covers H % 16 == 0 and W % 16 == 0 only (NCAHIP_ERANGE otherwise): there is no remainder grid to reach."""
    B, H, W = shape
    gch, Tn = C - 4, TN
    prm = rand_cond_prm(C, seed=950 + C, out_scale=1.0)
    gen = torch.Generator().manual_seed(9500 + C)
    x0 = torch.rand(B, C, H, W, generator=gen)
    x0[:, 3] *= 0.12
    x0, goal = x0.to(DEV), (torch.randn(B, gch, H, W, generator=gen) * 0.5).to(DEV)
    dr = Draws(ops, "philox" if C % 2 else "bits", B, H, W, Tn, 0.5, seed=PHILOX_KEY, gen_seed=C)
    w = _cond_w(ops, prm, x0)
    L, P = ops.lib(), ops._p
    nbytes = L.ncahip_cond_grow_persist_workspace(B, C, H, W, w.hidden, gch)
    assert nbytes > 0
    ws, epoch = ops._persist_workspace(nbytes, x0.device)
    states = torch.empty(Tn + 1, B, C, H, W, device=DEV)
    pre = torch.zeros(Tn + 1, B, H, W, device=DEV, dtype=torch.uint8)
    out = torch.empty_like(x0)
    states[0].copy_(x0)
    us, seed = ops._u_args(dr.arg, Tn, B, H, W, dr.seed)
    rc = L.ncahip_cond_grow_fwd_persist_f32(P(states), P(pre), Tn + 1, Tn, P(out), P(goal), gch, P(us), P(w.wp), P(w.w1), P(w.b1), P(w.w2),
                                            P(w.b2), P(w.w3), B, C, H, W, w.hidden, 3, 0.1, 0.5, -10.0, 10.0, seed, 0, P(ws), nbytes, epoch,
                                            ops._stream())
    assert rc == 0, rc
    ops.check_errors()
    worst, near, _ = _replay(states, pre, out, O.cond_pad_goal(goal.double(), C), dr, _f64(prm), 3, 0.5)
    ref = ops.cond_grow(x0, Tn, goal, dr.arg, w, 3, seed=dr.seed, keep_history=True)
    same = torch.equal(ref[0], out) and torch.equal(ref[1][1:], states[1:]) and torch.equal(ref[2][1:], pre[1:])
    _say(f"persistent grow C={C} {shape}", pre_mismatch=worst["pre"], nonfiring_changed=worst["keep"], firing_worst=worst["fire"],
         bound=REPLAY_TOL, final_mismatch=worst["final"], equals_per_step=same, near_threshold_cells_checked=near)
    assert worst["pre"] == 0 and worst["keep"] == 0 and worst["final"] == 0 and worst["fire"] <= REPLAY_TOL, worst
    assert same


# ================================================================================================ bf16 history
_BF16 = {}


def bf16_run(ops, ch, shape):
    """a bf16 row: the recorded bf16 history, the quiet cotangent on it and the kernel's exact-product gradients (force 4)"""
    if (ch, shape) in _BF16:
        return _BF16[ch, shape]
    (C, hid), (H, W), B, gch = BF16_CH[ch], BF16_SHAPES[shape], BF16_B[shape], BF16_CH[ch][0] - 4
    prm = rand_cond_prm(C, seed=970 + C + H, hidden=hid, out_scale=1.0)
    gen = torch.Generator().manual_seed(9700 + 10 * C + H)
    x0 = torch.rand(B, C, H, W, generator=gen)
    x0[:, 3] *= 0.12
    goal = torch.randn(B, gch, H, W, generator=gen) * 0.5
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    x0, goal = x0.to(DEV).bfloat16(), goal.to(DEV).bfloat16()
    dr = Draws(ops, ("uniform", "bits", "philox")[(C + H) % 3], B, H, W, TN, 0.5, seed=PHILOX_KEY, gen_seed=C + H)
    r = dict(case=f"bf16 {ch} {shape}", prm=prm, p64=_f64(prm), x0=x0, goal=goal, dr=dr, w=_cond_w(ops, prm, x0), Tn=TN, alive=3, rate=0.5,
             C=C, gch=gch, gpad=O.cond_pad_goal(goal.double(), C))
    r["out"], r["states"], r["pre"] = ops.cond_grow(x0, TN, goal, dr.arg, r["w"], 3, seed=dr.seed, keep_history=True)
    ops.check_errors()
    assert r["states"].dtype == torch.bfloat16
    r["cot"], r["gates_quiet"], r["zeroed"] = quiet_cotangent(cot, r["states"], r["pre"], r["gpad"], dr, r["p64"], 3, 0.5)
    _BF16[ch, shape] = r
    return r


@pytest.mark.parametrize("ch,shape", BF16_CASES)
def test_bf16_forward(ops, ch, shape):
    """launch_cond_pc<12|16|20, EXACT, StBF16>: test_gpu_cond_replay._bf16_case's criterion at these shapes (pre exact, pending within
    2 bf16 ulp of cond_step_bf16 from the GPU's own input, < 3 % of elements differing, final and ring 2 equal)"""
    r = bf16_run(ops, ch, shape)
    _bf16_case(ops, r["case"], r["prm"], r["x0"].float(), r["goal"].float(), TN, r["dr"])


@pytest.mark.parametrize("ch,shape", BF16_CASES)
def test_bf16_backward_exact_products(ops, ch, shape):
    """ncahip_cond_grow_bwd_bf16 with exact-f32 products (force bit 2): launch_bwd<12|16, StBF16> one launch (4 | 8 | 16) or
    launch_fm<12|16|20, StBF16, false> (4: split, 4 | 16: whole super-tiles), whose front kernel reads a uint16_t history; kernel B
    <float, 4>.  Against the FLOAT64 replay VJP at the recorded bf16 history widened to float64, GTOL, every element compared."""
    r = bf16_run(ops, ch, shape)
    ref = O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], r["p64"], r["cot"], 3)
    worst = {}
    for force in (4, 4 | 16, 4 | 8 | 16):
        e = _grad_errs(backward(ops, r, force), *ref, r["C"], r["gch"])
        worst[force] = max(e.values())
        for k, v in e.items():
            assert v < GTOL, (force, k, e)
    _say(r["case"] + " bwd exact products", **{f"force_{f}": v for f, v in worst.items()}, bound=GTOL,
         gates_within_4_GATE_K=r["gates_quiet"], cells_zeroed_fraction=r["zeroed"])


def _parts(ref, gch):
    """a float64 (dL/dx0, dL/dgoal_pad, {param: grad}) triple under the kernel's names"""
    return {"x0": ref[0], "goal": ref[1][:, -gch:], **{k: ref[2][n] for k, n in COND_NAMES.items()}}


@pytest.mark.parametrize("ch,shape", BF16_CASES)
def test_bf16_backward_mfma(ops, ch, shape):
    """The default bf16-history backward (products on bf16 MFMA: launch_fm<12|16|20, StBF16, true>, 8 waves at CP <= 16 and 4 at CP = 20,
    uint16_t stencil scratch, slot_order 1 in the unpermute) in both forms of kernel A (0: front + matrix; 8 | 16: one launch at
    C <= 16), with the bounds of test_cond_grow_backward_bf16_history, relative L2 per gradient.

    (iii) < 4e-2 (T = 3) against the function the kernel differentiates.  That test holds alpha fixed and compares with
    cond_grow_bf16_loss_grads free-running from x0; here alpha evolves and a free-running trajectory may resolve a life mask
    differently than the recorded one, so the same function is restarted from the recorded input of every step:
    cond_replay_vjp(bf16_operands=True), masks from the history (tests/test_oracle_replay_bf16.py ties the two).  The bound still
    applies: same gates, same operands, the kernel additionally rounds its gradient operands to bf16, and two trajectories that could
    drift apart have become one.

    (ii) < 8e-2 against the exact products of the same history (the kernel's own under force 4, and the float64 replay VJP).  This
    bound does NOT carry over to every row.  Measured on the CPU in float64 on cond_step_bf16 histories of these 18 rows, the
    bf16-operand VJP itself differs from the exact-product VJP by rho = 3.2e-2 .. 7.6e-2 (worst gradient per row, mostly b1 and w1:
    c9 4x16 7.6e-2, c18 5x20 7.0e-2; dL/dx0 4e-3 .. 1e-2), and more cells do not lower it.  The kernel cannot be closer to the exact
    products than the function it differentiates, so per gradient the bound is max(8e-2, rho + 4e-2): rho from the two float64
    references on the recorded history (printed), 4e-2 the margin that (iii) grants the kernel."""
    r = bf16_run(ops, ch, shape)
    ref_exact = _parts(O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], r["p64"], r["cot"], 3), r["gch"])
    ref_bf = _parts(O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], r["p64"], r["cot"], 3, bf16_operands=True), r["gch"])
    rho = {k: _rel2(ref_bf[k], ref_exact[k]) for k in ref_bf}
    gx = backward(ops, r, 4)
    for force in (0, 8 | 16):
        g = backward(ops, r, force)
        e_bf = {k: _rel2(g[k], ref_bf[k]) for k in g}
        e_ex = {k: max(_rel2(g[k], ref_exact[k]), _rel2(g[k], gx[k])) for k in g}
        kb, kx = max(e_bf, key=e_bf.get), max(e_ex, key=lambda k: e_ex[k] - max(8e-2, rho[k] + 4e-2))
        _say(r["case"] + f" bwd bf16 MFMA [force {force}]", vs_bf16_operands=e_bf[kb], of=kb, bound=4e-2, vs_exact=e_ex[kx], of_=kx,
             rho=rho[kx], bound_exact=max(8e-2, rho[kx] + 4e-2), rho_worst=max(rho.values()))
        for k in g:
            assert e_bf[k] < 4e-2, (force, k, e_bf)
            assert e_ex[k] < max(8e-2, rho[k] + 4e-2), (force, k, e_ex, rho)


# ================================================================================================ negative controls
def _last_wave_tile(H, W):
    """the last, partial 4 x 16 wave tile of an H x W grid"""
    return slice(4 * ((H - 1) // 4), H), slice(16 * ((W - 1) // 16), W)


def test_control_one_weight_entry(ops):
    """the reference with ONE output-layer weight entry scaled by 1 + 1e-3 must miss REPLAY_TOL and GTOL"""
    r = run(ops, "g16x16")       # the row whose float64 gradients move most under the change (6.9e-4 on the CPU; 1.9e-4 at g17x20)
    assert r["gates"] == 0, _pick("g16x16")
    bad, entry = _lever(r["prm"], r["states"], r["gpad"])
    worst, _, _ = _replay(r["states"], r["pre"], r["out"], r["gpad"], r["dr"], bad, 3, 0.5)
    e = _grad_errs(backward(ops, r, 0), *O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], bad, r["cot"], 3), r["C"], r["gch"])
    _say(f"control {entry} * (1 + 1e-3)", fwd_firing_worst=worst["fire"], fwd_bound=REPLAY_TOL, **e, bound=GTOL)
    assert worst["fire"] > REPLAY_TOL and max(e.values()) > GTOL


def test_control_wave_tile_cotangent(ops):
    """the reference cotangent zeroed on the last, partial wave tile (1 x 4 cells of 5 x 20) must miss GTOL in x0, and the bf16-MFMA rows'
    relative-L2 bounds in x0"""
    r = run(ops, "g5x20")
    assert r["gates"] == 0, _pick("g5x20")
    ys, xs = _last_wave_tile(5, 20)
    cot = r["cot"].clone()
    cot[:, :, ys, xs] = 0
    gx = O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], r["p64"], cot, 3)[0]
    e = _rmax(backward(ops, r, 0)["x0"], gx)
    b = bf16_run(ops, "c16", "5x20")
    cot = b["cot"].clone()
    cot[:, :, ys, xs] = 0
    g = backward(ops, b, 0)["x0"]
    e_exact = _rel2(g, O.cond_replay_vjp(b["states"], b["pre"], b["gpad"], b["dr"], b["p64"], cot, 3)[0])
    e_bf = _rel2(g, O.cond_replay_vjp(b["states"], b["pre"], b["gpad"], b["dr"], b["p64"], cot, 3, bf16_operands=True)[0])
    _say("control cotangent of the last wave tile zeroed", fp32_x0=e, bound=GTOL, mfma_x0_vs_exact=e_exact, bound_exact=8e-2,
         mfma_x0_vs_bf16_operands=e_bf, bound_bf16_operands=4e-2)
    assert e > GTOL and e_exact > 8e-2 and e_bf > 4e-2


def test_control_wrong_halo(ops):
    """the reference replayed with alive_ch = -1 on a row with an alive channel must miss the forward check: the row sees the life masks"""
    r = run(ops, "g17x20")
    worst, _, _ = _replay(r["states"], r["pre"], r["out"], r["gpad"], r["dr"], r["p64"], -1, 0.5)
    _say("control reference without an alive channel", nonfiring_changed=worst["keep"], firing_worst=worst["fire"], bound=REPLAY_TOL,
         final_mismatch=worst["final"])
    assert worst["fire"] > REPLAY_TOL and worst["keep"] > 0 and worst["final"] > 0


def test_control_lost_hidden_units(ops):
    """hidden = 40: the reference without the last 40 - 16 * floor(39 / 16) = 8 hidden units (a lost last 16-slice) must miss the bounds"""
    r = run(ops, "g2x4")
    assert r["gates"] == 0, _pick("g2x4")
    hid = CASES["g2x4"][2]
    keep = 16 * ((hid - 1) // 16)
    n = COND_NAMES
    p = dict(r["p64"])
    p[n["w1"]], p[n["b1"]] = p[n["w1"]][:keep], p[n["b1"]][:keep]
    p[n["w2"]], p[n["b2"]] = p[n["w2"]][:keep, :keep], p[n["b2"]][:keep]
    p[n["w3"]] = p[n["w3"]][:, :keep]
    worst, _, _ = _replay(r["states"], r["pre"], r["out"], r["gpad"], r["dr"], p, 3, 0.5)
    gx, gg, gw = O.cond_replay_vjp(r["states"], r["pre"], r["gpad"], r["dr"], p, r["cot"], 3)
    g = backward(ops, r, 0)
    e = {"x0": _rmax(g["x0"], gx), "wp": _rmax(g["wp"], gw[n["wp"]]), "w1": _rmax(g["w1"][:keep], gw[n["w1"]])}
    _say(f"control hidden units {keep}..{hid - 1} dropped", fwd_firing_worst=worst["fire"], fwd_bound=REPLAY_TOL, **e, bound=GTOL)
    assert worst["fire"] > REPLAY_TOL and min(e.values()) > GTOL


# ================================================================================================ the composed path, through the module
COMPOSED = {16: 41004, 20: 42001}       # C -> input seed: zero gates within SAFETY * GATE_K, no near-threshold cell (composed_search)


def composed_inputs(C, seed):
    B, H, W = 2, 5, 10
    prm = rand_cond_prm(C, seed=990 + C, out_scale=1.0)
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=gen)
    x0[:, 3] *= 0.12
    goal = torch.randn(B, C - 4, H, W, generator=gen) * 0.5
    cot = torch.randn(B, C, H, W, generator=gen)
    us = [torch.from_numpy(O.philox_uniform(PHILOX_KEY, k, B, H, W)) for k in range(TN)]
    return prm, x0, goal, cot, us


def composed_search(tries=100000):
    for C in COMPOSED:
        for seed in range(41000 + 1000 * (C == 20), 10 ** 6):
            prm, x0, goal, cot, us = composed_inputs(C, seed)
            p64 = {k: v.double() for k, v in prm.items()}
            gpad = O.cond_pad_goal(goal.double(), C)
            steps, _ = f64_trajectory(x0, gpad, us, p64, 3, 0.5)
            if any(bool(near_threshold(s).any()) for x, _, x1, _ in steps for s in (x, x1)):
                continue
            if int(O.cond_gate_influence(x0.double(), gpad, us, p64, 3, SAFETY * GATE_K)[1].sum()) == 0:
                print(f"COMPOSED[{C}] = {seed}", flush=True)
                break


@pytest.mark.parametrize("C", [16, 20])
def test_composed_path_through_the_module(ops, C, monkeypatch):
    """ConditionedNCA.grow under autograd at W = 10 takes ncahip.autograd._cond_grow_composed (asserted): every gradient against
    float64 autograd through the oracle from the same x0, GTOL, zero gates within GATE_K asserted"""
    from ncahip import autograd as AG
    from ncahip.nca import ConditionedNCA
    prm, x0, goal, cot, us = composed_inputs(C, COMPOSED[C])
    m = ConditionedNCA(encoder=torch.nn.Identity(), target_shape=(3, 5, 10), num_hidden_channels=C - 4, living_channel_dim=3).to(DEV)
    names = dict(COND_NAMES)
    with torch.no_grad():
        for n in names.values():
            dict(m.named_parameters())[n].copy_(prm[n])
    m.mask_rng, m.mask_seed, m._mask_step = "philox", PHILOX_KEY, 0
    calls, real = [], AG._cond_grow_composed
    monkeypatch.setattr(AG, "_cond_grow_composed", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    x = x0.to(DEV).requires_grad_(True)
    gl = goal.to(DEV).requires_grad_(True)
    out = m.grow(x, TN, gl)
    (out * cot.to(DEV)).sum().backward()
    assert calls == [1]
    p64 = _f64(prm)
    gpad = O.cond_pad_goal(goal.to(DEV).double(), C)
    us = [u.to(DEV) for u in us]
    assert int(O.cond_gate_influence(x0.to(DEV).double(), gpad, us, p64, 3, GATE_K)[1].sum()) == 0, "pick another seed (composed_search())"
    xT, gx, gg, gw = O.cond_grow_loss_grads(x0.to(DEV).double(), gpad, us, p64, 3, 0.1, 0.5, cot.to(DEV).double())
    e = {"out": _rel(out, xT), "x0": _rmax(x.grad, gx), "goal": _rmax(gl.grad, gg[:, 4:])}
    e.update({k: _rmax(dict(m.named_parameters())[n].grad, gw[n]) for k, n in names.items()})
    _say(f"composed path C={C} 2x{C}x5x10", **e, fwd_bound=REL_TOL, bound=GTOL)
    assert e.pop("out") < REL_TOL
    for k, v in e.items():
        assert v < GTOL, (k, e)


if __name__ == "__main__":
    torch.set_num_threads(8)
    if len(sys.argv) > 1 and sys.argv[1] == "composed":
        composed_search()
    else:
        search(sys.argv[1:] or None)
