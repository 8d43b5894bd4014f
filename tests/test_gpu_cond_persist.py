"""GPU tests of the one-launch persistent ConditionedNCA grow (ncahip_cond_grow_fwd_persist_f32, csrc/nca_cond_persist.hip).
Its contract is "the same numbers as the per-step producer/consumer kernels, bit for bit" -- x_final and, with history, every
states / pre slot -- so every case is checked with torch.equal against ops.persistent_cond = False on the same inputs, plus the
oracle directly at 1e-4."""
import random

import numpy as np
import pytest
import torch

from oracle import nca_oracle as O
from gpu_ops import gpu_ops
from util import REL_TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_cond=True) as o:
        o.check_errors()
        yield o


def _prm(C, seed, hidden=64, out_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=g) * 0.3,
            "update_net.out.0.weight": torch.randn(hidden, 3 * C, 1, 1, generator=g) * (1.0 / (3 * C) ** 0.5),
            "update_net.out.0.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.2.weight": torch.randn(hidden, hidden, 1, 1, generator=g) * (1.0 / hidden ** 0.5),
            "update_net.out.2.bias": torch.randn(hidden, generator=g) * 0.1,
            "update_net.out.4.weight": torch.randn(C, hidden, 1, 1, generator=g) * (out_scale * 0.3 / hidden ** 0.5)}


def _w(ops, prm, like):
    return ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                           prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], like)


class _Spy:
    """Wraps the persistent entry point of the loaded library and records its return codes."""

    def __init__(self, ops):
        self.L = ops.lib()
        self.orig = self.L.ncahip_cond_grow_fwd_persist_f32
        self.seen = []

    def __call__(self, *a):
        rc = self.orig(*a)
        self.seen.append(rc)
        return rc

    def __enter__(self):
        self.L.ncahip_cond_grow_fwd_persist_f32 = self
        return self

    def __exit__(self, *exc):
        self.L.ncahip_cond_grow_fwd_persist_f32 = self.orig


def _both(ops, x, Tn, goal, us, w, alive=3, hist=False, **kw):
    """(per-step result, persistent result), each (x_final, states, pre); asserts the persistent entry ran (rc 0)."""
    ops.persistent_cond = False
    ref = ops.cond_grow(x, Tn, goal, us, w, alive, keep_history=hist, **kw)
    ref = tuple(None if r is None else r.clone() for r in ref)
    ops.persistent_cond = True
    with _Spy(ops) as spy:
        got = ops.cond_grow(x, Tn, goal, us, w, alive, keep_history=hist, **kw)
    got = tuple(None if r is None else r.clone() for r in got)
    ops.check_errors()
    assert spy.seen == [0], spy.seen
    return ref, got


def _assert_same(ref, got, Tn, hist, what):
    assert torch.equal(ref[0], got[0]), (what, float((ref[0] - got[0]).abs().max()))
    if hist:
        for t in range(1, Tn + 1):
            assert torch.equal(ref[1][t], got[1][t]), (what, "states", t)
            assert torch.equal(ref[2][t], got[2][t]), (what, "pre", t)
    else:
        assert got[1] is None and got[2] is None


def _straddle(x, alive, thr=0.1, gen=None):
    """alpha within +-1e-3 of the threshold on the rows / columns at every 16-cell tile edge (the alpha halo-3 / pre halo-2 cone)"""
    B, C, H, W = x.shape
    edge = torch.zeros(H, W, dtype=torch.bool)
    for k in range(0, H, 16):
        edge[max(k - 2, 0):k + 2, :] = True
    for k in range(0, W, 16):
        edge[:, max(k - 2, 0):k + 2] = True
    jit = (torch.rand(B, H, W, generator=gen) * 2 - 1) * 1e-3
    x = x.clone()
    x[:, alive][:, edge] = (thr + jit)[:, edge]
    return x


@pytest.mark.parametrize("C", [12, 16, 20])
@pytest.mark.parametrize("shape", [(1, 64, 64), (8, 64, 64), (2, 32, 96), (1, 256, 256)])
def test_persistent_grow_equals_per_step_bit_for_bit(ops, C, shape):
    B, H, W = shape
    gen = torch.Generator().manual_seed(C * 7 + H + B)
    prm = _prm(C, seed=C + B, out_scale=2.0)
    xr = torch.rand(B, C, H, W, generator=gen) * 0.4 - 0.1
    x = _straddle(xr, 3, gen=gen).to(DEV)
    w = _w(ops, prm, x)
    gch = C - 4
    goal = (torch.randn(B, gch, H, W, generator=gen) * 0.5).to(DEV)
    cases = [(1, "bits", True, True), (2, "philox", False, True), (7, "bits", True, False), (64, "philox", True, True),
             (7, "philox", False, False), (2, "bits", True, False)]
    if B * H * W > 64 * 64 * 2:
        cases = cases[:4]
    assert ops.lib().ncahip_cond_grow_persist_workspace(B, C, H, W, 64, gch) > 0
    for Tn, mode, with_goal, hist in cases:
        us = None
        if mode == "bits":
            us = ops.pack_fire_mask(torch.rand(Tn, B, 1, H, W, generator=gen).to(DEV), 0.5, "cond")
        g = goal if with_goal else None
        ref, got = _both(ops, x, Tn, g, us, w, 3, hist, seed=17 + Tn, step0=3)
        _assert_same(ref, got, Tn, hist, (C, shape, Tn, mode, with_goal, hist))


def test_backward_consumes_the_persistent_history(ops):
    """ncahip_cond_grow_bwd_f32 on the persistent grow's history gives every gradient bit for bit as on the per-step history."""
    gen = torch.Generator().manual_seed(12)
    B, C, H, W, Tn = 8, 20, 64, 64, 7
    prm = _prm(C, seed=13, out_scale=2.0)
    x = _straddle(torch.rand(B, C, H, W, generator=gen) * 0.4 - 0.1, 3, gen=gen).to(DEV)
    goal = (torch.randn(B, 16, H, W, generator=gen) * 0.5).to(DEV)
    us = ops.pack_fire_mask(torch.rand(Tn, B, 1, H, W, generator=gen).to(DEV), 0.5, "cond")
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    w = _w(ops, prm, x)
    ref, got = _both(ops, x, Tn, goal, us, w, 3, True)
    gr = ops.cond_grow_backward(ref[1], ref[2], goal, us, w, cot, Tn, 3)
    gg = ops.cond_grow_backward(got[1], got[2], goal, us, w, cot, Tn, 3)
    for k in gr:
        assert (gr[k] is None and gg[k] is None) or torch.equal(gr[k], gg[k]), k


def test_seed_front_crosses_tile_borders(ops):
    """A grow from generate_seed: the seed sits on the corner of four 16 x 16 tiles, so its living front crosses tile borders
    from the first step on."""
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(4)
    m = ConditionedNCA().to(DEV)
    x = m.generate_seed(8).to(DEV)
    prm = _prm(m.num_channels, seed=2, out_scale=3.0)
    w = _w(ops, prm, x)
    goal = (torch.randn(8, 16, 64, 64) * 0.5).to(DEV)
    for hist in (False, True):
        ref, got = _both(ops, x, 64, goal, None, w, 3, hist, seed=9)
        _assert_same(ref, got, 64, hist, ("seed", hist))
    alive = ops.cond_alive(got[1][1], 3)[:, 0]
    assert bool(alive[:, 31, 31].all() and alive[:, 32, 32].all() and alive[:, 31, 32].all() and alive[:, 32, 31].all())


def test_no_alive_channel(ops):
    gen = torch.Generator().manual_seed(3)
    x = (torch.rand(2, 16, 64, 64, generator=gen) - 0.5).to(DEV)
    w = _w(ops, _prm(16, seed=8), x)
    ref, got = _both(ops, x, 7, None, None, w, -1, True, seed=2)
    _assert_same(ref, got, 7, True, "alive -1")


def test_persistent_grow_vs_oracle(ops):
    B, C, H, W, Tn = 2, 20, 32, 32, 4
    prm = _prm(C, seed=5, out_scale=0.5)
    gen = torch.Generator().manual_seed(6)
    x0 = torch.rand(B, C, H, W, generator=gen)
    goal = torch.randn(B, 16, H, W, generator=gen) * 0.5
    us = torch.rand(Tn, B, 1, H, W, generator=gen)
    ref = O.cond_grow(x0, O.cond_pad_goal(goal, C), list(us), prm, 3)
    w = _w(ops, prm, x0.to(DEV))
    bits = ops.pack_fire_mask(us.to(DEV), 0.5, "cond")
    with _Spy(ops) as spy:
        got, _, _ = ops.cond_grow(x0.to(DEV), Tn, goal.to(DEV), bits, w, 3)
    assert spy.seen == [0]
    assert rel_err(got.cpu(), ref) < REL_TOL


def _same_params(ref, got):
    """{name: tensor}: bit-equal for the NCA's own parameters (their gradients come from ncahip_cond_grow_bwd_f32 on the grow's
    history); the goal encoder's gradients also pass through torch's convolution backward, which is not guaranteed to be
    run-to-run bit-reproducible, so those are compared at 1e-5 of their scale."""
    assert ref.keys() == got.keys() and len(ref) > 0
    own = 0
    for n, a in ref.items():
        b = got[n]
        if n.startswith("encoder."):
            assert float((a - b).abs().max()) <= 1e-5 * max(float(a.abs().max()), 1e-12), n
        else:
            assert torch.equal(a, b), n
            own += 1
    assert own > 0


def test_module_grow_runs_the_persistent_kernel(ops):
    """ConditionedNCA() (C = 20) grow at 8 x 64^2: no_grad and autograd go through the persistent launch, with the same output
    and the same parameter gradients as the per-step kernels."""
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(1)
    m = ConditionedNCA().to(DEV)
    assert m.num_channels == 20
    x = m.generate_seed(8).to(DEV)
    img = torch.rand(8, 3, 64, 64, device=DEV)

    def run(persist, grad):
        ops.persistent_cond = persist
        m.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        if grad:
            out = m.grow(x, 24, img)
            (out.float().pow(2).mean() + out[:, :4].sum() * 1e-3).backward()
            return out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        with torch.no_grad():
            return m.grow(x, 24, img).clone(), {}
    try:
        for grad in (False, True):
            ref, gref = run(False, grad)
            with _Spy(ops) as spy:
                got, ggot = run(True, grad)
            assert spy.seen == [0], spy.seen
            assert torch.equal(ref, got)
            if grad:
                _same_params(gref, ggot)
    finally:
        ops.persistent_cond = True
    ops.check_errors()


def test_trainer_iteration_runs_the_persistent_kernel(ops):
    """One ConditionedNCATrainer iteration (the stand-in loss of test_gpu_modules) goes through the persistent launch.  The
    iteration's second batch already sees the goal encoder updated by the first, and the encoder's gradient passes through torch's
    convolution backward (not run-to-run bit-reproducible), so the parameters after the step are compared at 1e-5; the grow and
    its backward themselves are pinned bit for bit above."""
    from ncahip.conditioned_trainer import ConditionedNCATrainer
    from ncahip.nca import ConditionedNCA

    class DS:
        target_size = (3, 64, 64)

        def __init__(self):
            self.x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(0))

        def __len__(self):
            return 8

        def __getitem__(self, i):
            return self.x[i]

    class PixLoss(torch.nn.Module):
        def forward(self, d):
            s = d["nca_state"].float()
            l = (d["generated_images"].float() - d["target_images"]).pow(2).mean() + (s - s.clamp(-1, 1)).abs().mean()
            return [l, {"pix": l.detach()}]

    def run(persist):
        ops.persistent_cond = persist
        torch.manual_seed(3)
        m = ConditionedNCA().to(DEV)
        tr = ConditionedNCATrainer(m, DS(), None, nca_steps=[8, 12], lr=2e-3, pool_size=16, log_base_path="/tmp/ncahip_gpu_test",
                                   loss=PixLoss(), device=torch.device(DEV))
        random.seed(0); np.random.seed(0); torch.manual_seed(0)
        tr.train(batch_size=8, epochs=1)
        return {n: p.detach().clone() for n, p in m.named_parameters()}
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        ref = run(False)
        with _Spy(ops) as spy:
            got = run(True)
    finally:
        ops.persistent_cond = True
        torch.backends.cudnn.deterministic = det
    assert spy.seen and all(rc == 0 for rc in spy.seen), spy.seen
    assert ref.keys() == got.keys()
    for n, a in ref.items():
        assert torch.allclose(a, got[n], rtol=1e-5, atol=1e-5), (n, float((a - got[n]).abs().max()))
    ops.check_errors()


def _fallback(ops, x, Tn, goal, w, expect, **kw):
    """the persistent entry refuses (ERANGE) or is never called, and the result is the per-step family's"""
    from ncahip import _capi
    ops.persistent_cond = False
    ref = ops.cond_grow(x, Tn, goal, None, w, 3, seed=4, **kw)[0].clone()
    ops.persistent_cond = True
    with _Spy(ops) as spy:
        got = ops.cond_grow(x, Tn, goal, None, w, 3, seed=4, **kw)[0].clone()
    if expect == "erange":
        assert spy.seen == [_capi.ERANGE], spy.seen
    else:
        assert spy.seen == [], spy.seen
    assert torch.equal(ref, got)


def test_fallbacks(ops):
    gen = torch.Generator().manual_seed(8)
    prm = _prm(16, seed=3)
    x = (torch.rand(2, 16, 64, 64, generator=gen) * 0.4).to(DEV)
    goal = (torch.randn(2, 12, 64, 64, generator=gen) * 0.5).to(DEV)
    w = _w(ops, prm, x)
    try:
        for bits in (1, 2, 8):
            ops.force_generic(bits)
            _fallback(ops, x, 5, goal, w, "erange")
        ops.force_generic(0)
        ops.set_cond_precision(1)
        _fallback(ops, x, 5, goal, w, "erange")
    finally:
        ops.force_generic(0)
        ops.set_cond_precision(0)
    _fallback(ops, x.to(torch.bfloat16), 5, goal.to(torch.bfloat16), w, "not called")          # bf16 state
    x40 = (torch.rand(2, 16, 40, 64, generator=gen) * 0.4).to(DEV)
    _fallback(ops, x40, 5, None, w, "not called")                                                # H = 40: workspace query 0
    x256 = (torch.rand(8, 16, 256, 256, generator=gen) * 0.4).to(DEV)
    _fallback(ops, x256, 2, None, w, "erange")                                                  # 2048 tiles
    # explicit float uniforms: per-step kernels
    us = torch.rand(3, 2, 1, 64, 64, generator=gen).to(DEV)
    ops.persistent_cond = False
    ref = ops.cond_grow(x, 3, goal, us, w, 3)[0].clone()
    ops.persistent_cond = True
    with _Spy(ops) as spy:
        got = ops.cond_grow(x, 3, goal, us, w, 3)[0].clone()
    assert torch.equal(ref, got) and spy.seen in ([], [-2])
    ops.check_errors()


# (the graph-capture test of this module lives in test_gpu_graph_replay.py: test_graph_capture_takes_the_per_step_kernels)


def test_epochs_interleaved_with_dynca_persistent(ops):
    """50 consecutive grows on one workspace (every call a new epoch), interleaved with persistent DyNCA launches on the same
    stream: each bit-equal to the per-step result."""
    gen = torch.Generator().manual_seed(10)
    x = (torch.rand(1, 20, 64, 64, generator=gen) * 0.4).to(DEV)
    goal = (torch.randn(1, 16, 64, 64, generator=gen) * 0.5).to(DEV)
    w = _w(ops, _prm(20, seed=6), x)
    g = torch.Generator().manual_seed(11)
    dprm = {"w1": torch.randn(96, 51, 1, 1, generator=g) * 0.07, "b1": torch.randn(96, generator=g) * 0.1,
            "w2": torch.randn(12, 96, 1, 1, generator=g) * 0.03, "b2": torch.randn(12, generator=g) * 0.02}
    xd = (torch.rand(1, 12, 64, 64, generator=g) - 0.5).to(DEV)
    cond = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    wd = ops.DyncaWeights(dprm["w1"], dprm["b1"], dprm["w2"], dprm["b2"], xd)
    ops.persistent_cond = False
    refs = [ops.cond_grow(x, 3 + i % 5, goal, None, w, 3, seed=i)[0].clone() for i in range(5)]
    ops.persistent_cond = True
    ops.persistent_steps = True
    dref = ops.dynca_nsteps(xd, 4, cond, None, wd, "circular", 0.5, seed=1)[0].clone()
    with _Spy(ops) as spy:
        for i in range(50):
            got = ops.cond_grow(x, 3 + i % 5, goal, None, w, 3, seed=i % 5)[0]
            assert torch.equal(got, refs[i % 5]), i
            d = ops.dynca_nsteps(xd, 4, cond, None, wd, "circular", 0.5, seed=1)[0]
            assert torch.equal(d, dref), i
    assert spy.seen == [0] * 50
    ops.check_errors()


def test_sticky_error_refuses_and_check_errors_names_the_switch(ops):
    """Through ncahip_debug_inject_error only: a set word refuses the persistent entry with the per-step driver's message, and
    bit 1 (an expired neighbour poll) is reported naming ops.persistent_cond."""
    from ncahip._capi import EDEVICE, NcaHipError
    x = (torch.rand(1, 16, 32, 32) * 0.4).to(DEV)
    w = _w(ops, _prm(16, seed=1), x)
    ops.check_errors()
    assert ops.lib().ncahip_debug_inject_error(2) == 0
    try:
        with _Spy(ops) as spy:
            with pytest.raises(NcaHipError, match="hand-off"):
                ops.cond_grow(x, 2, None, None, w, 3)
        assert spy.seen == [EDEVICE]
        with pytest.raises(NcaHipError, match="persistent_cond = False"):
            ops.check_errors()
    finally:
        ops.lib().ncahip_check_errors(ops._stream(), 1)      # never leave the word set for later tests
    ops.check_errors()
    out, _, _ = ops.cond_grow(x, 2, None, None, w, 3)
    assert bool(torch.isfinite(out).all())
