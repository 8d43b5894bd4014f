"""ops.reset_modes() on the device: results after it equal those of the default state bit for bit, and the persistent ConditionedNCA
grow runs again -- also in a process whose environment sets only BACKWARD modes (csrc/nca_modes.h: nca_cond_fwd_default)."""
import os
import subprocess
import sys

import pytest
import torch

from gpu_ops import gpu_ops
from test_gpu_configs import rand_cond_prm, rand_dynca_prm

pytestmark = pytest.mark.gpu
DEV = "cuda"
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "video-stylization-with-nca_amd")
T = 2


@pytest.fixture(scope="module")
def ops():
    with gpu_ops() as o:
        yield o
        o.check_errors()


def _cond_case(ops):
    """ConditionedNCA at 1 x 16 x 16 x 16, hidden 64, Philox masks: (x, goal, weights)"""
    C = 16
    prm = rand_cond_prm(C, seed=3)
    gen = torch.Generator().manual_seed(4)
    x = torch.rand(1, C, 16, 16, generator=gen).to(DEV)
    goal = (torch.randn(1, 12, 16, 16, generator=gen) * 0.5).to(DEV)
    w = ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                        prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], x)
    return x, goal, w


def persist_grow_rc(ops):
    """return code of ncahip_cond_grow_fwd_persist_f32 on real tensors (one tile, T = 2, no history)"""
    x, goal, w = _cond_case(ops)
    B, C, H, W = x.shape
    L, p = ops.lib(), ops._p
    nbytes = L.ncahip_cond_grow_persist_workspace(B, C, H, W, w.hidden, goal.shape[1])
    assert nbytes > 0
    ws, epoch = ops._persist_workspace(nbytes, x.device)
    out = torch.empty_like(x)
    rc = L.ncahip_cond_grow_fwd_persist_f32(p(x), None, 2, T, p(out), p(goal), goal.shape[1], None, p(w.wp), p(w.w1), p(w.b1), p(w.w2), p(w.b2),
                                            p(w.w3), B, C, H, W, w.hidden, 3, 0.1, 0.5, -10.0, 10.0, 1, 0, p(ws), nbytes, epoch,
                                            ops._stream())
    ops.check_errors()
    return rc


def _results(ops):
    """(cond_grow output, its fire-word launches, dynca_nsteps output) in whatever state the modes are"""
    x, goal, w = _cond_case(ops)
    grown = ops.cond_grow(x, T, goal, None, w, 3, seed=1)[0].clone()
    launches = ops.fire_word_launches()
    C, fc = 12, 96
    prm = rand_dynca_prm(C, fc, 0, seed=5)
    xd = (torch.rand(1, C, 16, 16, generator=torch.Generator().manual_seed(6)) - 0.5).to(DEV)
    wd = ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], xd)
    stepped = ops.dynca_nsteps(xd, T, None, None, wd, "circular", 0.5, seed=1)[0].clone()
    ops.check_errors()
    return grown, launches, stepped


def test_reset_modes_restores_the_default_results(ops):
    before = _results(ops)
    dirs = torch.zeros(1, 2, 16, 16, device=DEV)
    ops.force_generic(1 | 2 | 4 | 8 | 16 | 32 | 64 | 128 | (3 << 8) | (1 << 16))
    ops.set_cond_precision("bf16x3")
    ops.set_dynca_precision("bf16")
    ops._attach_direction(dirs)
    assert ops.lib().ncahip_debug_persist_drop_tiles(3) == 0
    ops.persistent_steps, ops.persistent_cond = False, True
    ops.reset_modes()
    after = _results(ops)
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2])
    assert before[1] == after[1]
    assert persist_grow_rc(ops) == 0            # nothing set: the persistent grow runs


def test_backward_environment_leaves_the_persistent_grow_alone():
    """NCAHIP_BWD_VARIANT / NCAHIP_BWD_BF16_EXACT are read when the library is loaded: a fresh process"""
    code = (f"import sys; sys.path[:0] = [{TESTS!r}, {ROOT!r}, {PKG!r}]; import test_gpu_modes as m; from ncahip import ops; "
            "ops.selftest(); print('rc', m.persist_grow_rc(ops))")
    env = dict(os.environ, NCAHIP_BWD_VARIANT="2", NCAHIP_BWD_BF16_EXACT="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rc 0" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
