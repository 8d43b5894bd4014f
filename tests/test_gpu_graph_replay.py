"""Captured graphs of the step drivers, replayed over changing inputs, against the same calls made eagerly.

A capture freezes pointers, seeds, epochs and the process-wide modes of its enqueue time into kernel arguments while the data changes
underneath; what a driver leaves behind for its next run -- ring slots, the per-tile step counters and the fire-word scratch a
fused-steps grow keeps inside x_final, cached workspaces -- is met again by every replay.  Every row runs through `replayed`: inputs in
static device buffers, three variants V0, V1, V2 from literal seeds, eager references first (V1 twice: the determinism precondition),
one eager warm-up on the capturing stream, ONE graph of one stream, the path facts asserted before any replay, then the replays V1, V2,
V1, V0, every output compared bit for bit (integer views: NaN and the sign of zero count).  A replay enqueues the same kernels with
the same arguments as the eager call, so equality is the contract and no tolerance appears in this file.

The persistent launches take their epoch as a kernel argument and are never part of a capture (include/ncahip.h): the rows that switch
them on assert that neither a persistent entry point nor ops._persist_workspace is reached while capturing."""
import contextlib

import pytest
import torch

from gpu_ops import gpu_ops
from test_gpu_clip_cond import _encoder, _weights as _clip_cond_weights
from test_gpu_fused_steps import NO_FUSED, ONE, _bits, _expected_launches, _inputs, _prm as _cond_prm, _w as _cond_w
from test_gpu_persist import _prm as _dynca_prm

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDER = (1, 2, 1, 0)      # every replay meets what a replay of OTHER data left behind, and the first differs from the warm-up (V0)
PERSIST_ENTRIES = ("ncahip_dynca_nsteps_fwd_persist_f32", "ncahip_dynca_nsteps_fwd_persist_ms_f32", "ncahip_cond_grow_fwd_persist_f32")


class _Spy:
    """Wraps the three persistent entry points of the loaded library (seen: (name, rc) of every call made from Python) and
    ops._persist_workspace (epochs: how many calls asked for epochs -- the C clip drivers call the entry points themselves, so for
    them the request for a workspace is what tells)."""

    def __init__(self, ops):
        self.ops, self.L = ops, ops.lib()
        self.orig = {n: getattr(self.L, n) for n in PERSIST_ENTRIES}
        self.orig_ws = ops._persist_workspace
        self.seen, self.epochs = [], 0

    def _entry(self, name):
        def call(*a):
            rc = self.orig[name](*a)
            self.seen.append((name, rc))
            return rc
        return call

    def _ws(self, *a, **kw):
        self.epochs += 1
        return self.orig_ws(*a, **kw)

    def __enter__(self):
        for n in PERSIST_ENTRIES:
            setattr(self.L, n, self._entry(n))
        self.ops._persist_workspace = self._ws
        return self

    def __exit__(self, *exc):
        for n in PERSIST_ENTRIES:
            setattr(self.L, n, self.orig[n])
        self.ops._persist_workspace = self.orig_ws


def _iv(t):
    """the integer view of a tensor: equality of these is equality of every bit"""
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    assert t.dtype in (torch.uint8, torch.int32, torch.int64), t.dtype
    return t


def _same_bits(got, want, tag):
    assert len(got) == len(want) and len(got) > 0, tag
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, tuple(a.shape), tuple(b.shape))
        assert torch.equal(_iv(a.contiguous()), _iv(b.contiguous())), (tag, "output", k, int((_iv(a.contiguous()) != _iv(b.contiguous())).sum()))


def _differ(a, b):
    return any(not torch.equal(_iv(p.contiguous()), _iv(q.contiguous())) for p, q in zip(a, b))


def _no_persistent_launch(spy):
    assert spy.seen == [] and spy.epochs == 0, (spy.seen, spy.epochs)


def replayed(ops, fn, statics, variants, path_facts=_no_persistent_launch, mode=contextlib.nullcontext, differs_without_mode=False,
             repeat_control=False):
    """fn() reads only the tensors of `statics` (name -> device tensor) and returns a tuple of output tensors; variants = [V0, V1, V2],
    each name -> tensor of the same shape.  mode: a context entered for the eager references, the warm-up and the capture and LEFT before
    the first replay (a process-wide mode is snapshotted when a call enqueues); differs_without_mode: after the replays the eager call
    without the mode gives other bits than the replay did.  path_facts(spy) is asserted after the capture and before any replay.
    Returns (the eager references, clones of the outputs after the last replay, which is V0's)."""
    assert len(variants) == 3 and all(v.keys() == statics.keys() for v in variants)

    def load(v):
        for k, t in statics.items():
            assert t.shape == v[k].shape and t.dtype == v[k].dtype, k
            t.copy_(v[k])

    def eager():
        return tuple(o.clone() for o in fn())

    with mode():
        refs = []
        for v in variants:
            load(v)
            refs.append(eager())
        load(variants[1])
        _same_bits(eager(), refs[1], "the eager call twice on V1: the driver is not deterministic, a finding of its own")
        assert _differ(refs[1], refs[2]), "V1 and V2 give the same outputs: the inputs do not matter"
        load(variants[0])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn()                                   # warm-up on the capturing stream: workspaces, the error word, cached tables, attributes
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with _Spy(ops) as spy:
            with torch.cuda.graph(g, stream=s):
                outs = tuple(fn())
        facts = ops.fused_step_launches(), ops.fire_word_launches()      # set at enqueue time
        path_facts(spy)
    try:
        for n, i in enumerate(ORDER):
            load(variants[i])
            g.replay()
            torch.cuda.synchronize()
            _same_bits(outs, refs[i], ("replay", n, "variant", i))
            if repeat_control and n == 0:          # nothing but the static buffers feeds a replay
                before = tuple(o.clone() for o in outs)
                g.replay()
                torch.cuda.synchronize()
                _same_bits(outs, before, "a replay without rewriting the buffers")
        assert (ops.fused_step_launches(), ops.fire_word_launches()) == facts       # a replay enqueues nothing through the drivers
        last = tuple(o.clone() for o in outs)
        if differs_without_mode:
            assert _differ(eager(), last), "the mode of the capture made no difference"
    finally:
        del g
    ops.check_errors()
    return refs, last


# ------------------------------------------------------------------------------------------------------------------ DyNCA
DC, DFC, DCC, DH, DW, DT, DPAD = 12, 96, 3, 32, 32, 3, "circular"      # four 16 x 16 tiles: the persistent kernel covers it


def _dynca_variants(C, cc, B, H, W, T, seed, dtype=torch.float32):
    out = []
    for k in range(3):
        g = torch.Generator().manual_seed(seed + 101 * k)
        v = {"x": (torch.rand(B, C, H, W, generator=g) - 0.5).to(DEV).to(dtype), "u": torch.rand(T, B, 1, H, W, generator=g).to(DEV),
             "cot": torch.randn(B, C, H, W, generator=g).to(DEV)}
        if cc:
            v["cond"] = (torch.rand(B, cc, H, W, generator=g) * 2 - 1).to(DEV)
        out.append(v)
    return out


def _statics(variants, names):
    picked = [{k: v[k] for k in names if k in v} for v in variants]
    return {k: torch.empty_like(t) for k, t in picked[0].items()}, picked


def _dynca_w(ops, C, fc, cc, seed, like):
    prm = _dynca_prm(C, fc, cc, seed, scale=2.0)
    return ops.DyncaWeights(prm["w1.weight"], prm["w1.bias"], prm["w2.weight"], prm["w2.bias"], like)


def _dynca_row(ops, masks="philox", two_scale=False, dtype=torch.float32, geo=(DC, DFC, DCC, 1, DH, DW), seed=3, ring=True, **kw):
    """ops.dynca_nsteps without history: the final state and both ring slots (T = 3: every slot is written).  ring=False: the final state
    alone -- all that an eager call on the persistent launch defines."""
    C, fc, cc, B, H, W = geo
    variants = _dynca_variants(C, cc, B, H, W, DT, seed, dtype)
    if masks == "bits":
        for v in variants:
            v["u"] = ops.pack_fire_mask(v["u"], 0.5, "dynca")
    S, variants = _statics(variants, ("x", "cond") + (() if masks == "philox" else ("u",)))
    w = _dynca_w(ops, C, fc, cc, seed + 1, S["x"])

    def fn():
        out, states = ops.dynca_nsteps(S["x"], DT, S.get("cond"), S.get("u"), w, DPAD, 0.5, seed=77, step0=5, two_scale=two_scale)
        return (out, states) if ring else (out,)
    return fn, replayed(ops, fn, S, variants, **kw)


def test_d1_per_step_philox_and_the_replay_controls():
    with gpu_ops(persistent_steps=False) as ops:
        _dynca_row(ops, repeat_control=True)


@pytest.mark.parametrize("masks", ["uniforms", "bits"])
def test_d2_explicit_masks_are_static_inputs(masks):
    with gpu_ops(persistent_steps=False) as ops:
        _dynca_row(ops, masks=masks, seed=5)


def test_d3_two_scale_per_step():
    with gpu_ops(persistent_steps=False) as ops:
        _dynca_row(ops, two_scale=True, seed=7)


@pytest.mark.parametrize("two_scale", [False, True])
def test_d4_persistent_steps_stay_out_of_the_capture(two_scale):
    """With ops.persistent_steps on, the eager calls take the one-launch kernel (bit-equal to the per-step kernels by its contract); the
    capture takes the per-step kernels without asking for a workspace or an epoch, and the eager call after the replays is persistent
    again."""
    with gpu_ops(persistent_steps=True) as ops:
        assert ops.lib().ncahip_dynca_nsteps_persist_workspace(1, DC, DH, DW, DFC, DCC) > 0
        fn, (refs, _) = _dynca_row(ops, two_scale=two_scale, seed=9, ring=False)
        with _Spy(ops) as spy:
            again = tuple(o.clone() for o in fn())                       # the static buffers hold V0
        assert spy.seen == [(PERSIST_ENTRIES[1 if two_scale else 0], 0)] and spy.epochs == 1, (spy.seen, spy.epochs)
        _same_bits(again, refs[0], "the persistent call after the replays")
        ops.check_errors()


def test_d4_persistent_entry_points_refuse_a_capturing_stream():
    """ncahip_dynca_nsteps_fwd_persist_f32 / _ms_f32 and ncahip_cond_grow_fwd_persist_f32 called directly: rc 0 eagerly, NCAHIP_ERANGE
    with a message that names the capture on a capturing stream (nothing of them is in the graph, which is never replayed)."""
    from ncahip import _capi
    from ncahip.ops import _p, _stream
    with gpu_ops() as ops:
        L = ops.lib()
        v = _dynca_variants(DC, DCC, 1, DH, DW, DT, 11)[0]
        w = _dynca_w(ops, DC, DFC, DCC, 12, v["x"])
        nb = L.ncahip_dynca_nsteps_persist_workspace(1, DC, DH, DW, DFC, DCC)
        ws, out = torch.zeros(nb, device=DEV, dtype=torch.uint8), torch.empty_like(v["x"])
        xc, goal = _inputs(1, 16, 16, 16, 13)
        cw = _cond_w(ops, _cond_prm(16, 13), xc)
        cnb = L.ncahip_cond_grow_persist_workspace(1, 16, 16, 16, 64, 12)
        cws, cout = torch.zeros(cnb, device=DEV, dtype=torch.uint8), torch.empty_like(xc)
        assert nb > 0 and cnb > 0

        def dynca(name, epoch):
            return getattr(L, name)(_p(v["x"]), _p(out), DT, _p(v["cond"]), None, _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), 1, DC, DH, DW, DFC, DCC,
                                    _capi.PAD_MODES[DPAD], 0.5, 77, 5, _p(ws), nb, epoch, _stream())

        def cond(epoch):
            return L.ncahip_cond_grow_fwd_persist_f32(_p(xc), None, 2, DT, _p(cout), _p(goal), 12, None, _p(cw.wp), _p(cw.w1), _p(cw.b1), _p(cw.w2),
                                                      _p(cw.b2), _p(cw.w3), 1, 16, 16, 16, 64, 3, 0.1, 0.5, -10.0, 10.0, 5, 0, _p(cws), cnb, epoch,
                                                      _stream())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                       # the same arguments are accepted outside a capture
            assert [dynca(PERSIST_ENTRIES[0], 1), dynca(PERSIST_ENTRIES[1], 2), cond(1)] == [0, 0, 0], L.ncahip_last_error()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g, seen = torch.cuda.CUDAGraph(), []
        with torch.cuda.graph(g, stream=s):
            filler = out.new_zeros(4) + 1                                # the graph is not empty
            for call in (lambda: dynca(PERSIST_ENTRIES[0], 3), lambda: dynca(PERSIST_ENTRIES[1], 4), lambda: cond(2)):
                seen.append((call(), (L.ncahip_last_error() or b"").decode()))
        del g, filler
        for rc, msg in seen:
            assert rc == _capi.ERANGE and "captur" in msg, (rc, msg)
        ops.check_errors()


def test_d5_bf16_state_storage():
    with gpu_ops(persistent_steps=False) as ops:
        _dynca_row(ops, dtype=torch.bfloat16, seed=15)


@pytest.mark.parametrize("precision,geo", [("bf16", (DC, DFC, DCC, 1, DH, DW)), ("bf16_wide", (20, 160, 2, 1, 16, 16))])
def test_d6_dynca_precision_is_snapshotted_at_enqueue(precision, geo):
    """the ambient precision of the capture is back at 'f32' before the first replay: the replays still give the bf16-MFMA bits"""
    with gpu_ops(persistent_steps=False) as ops:
        assert ops.dynca_bf16_ok(geo[0], geo[1]) == (precision == "bf16") and ops.dynca_bf16_wide_ok(geo[0], geo[1])
        _dynca_row(ops, geo=geo, seed=17, mode=lambda: ops.dynca_precision(precision), differs_without_mode=True)


def test_d7_direction_field_is_snapshotted_at_enqueue():
    """the field is detached before the first replay; its tensor stays alive and unchanged, and the replays are steered"""
    from ncahip import steer
    with gpu_ops(persistent_steps=False) as ops:
        field = steer.direction_field("polar", 30.0, DH, DW, DEV)
        kept = field.clone()
        _dynca_row(ops, seed=19, mode=lambda: ops.dynca_direction(field), differs_without_mode=True)
        assert torch.equal(field, kept)


@pytest.mark.parametrize("two_scale,precision,geo", [(False, "f32", (DC, DFC, DCC, 1, DH, DW)), (True, "f32", (DC, DFC, DCC, 1, DH, DW)),
                                                     (False, "bf16", (12, 96, 3, 1, 16, 16))])      # the last: row "a" of test_dynca_train_bf16_host
def test_d8_history_forward_and_backward_in_one_capture(two_scale, precision, geo):
    C, fc, cc, B, H, W = geo
    with gpu_ops(persistent_steps=False) as ops:
        S, variants = _statics(_dynca_variants(C, cc, B, H, W, DT, 21), ("x", "cond", "cot"))
        w = _dynca_w(ops, C, fc, cc, 22, S["x"])

        def fn():
            with ops.dynca_precision(precision):
                out, states = ops.dynca_nsteps(S["x"], DT, S["cond"], None, w, DPAD, 0.5, seed=31, step0=2, keep_history=True, two_scale=two_scale)
            g = ops.dynca_nsteps_backward(states, S["cond"], None, w, S["cot"], None, DT, DPAD, 0.5, seed=31, step0=2, two_scale=two_scale,
                                          precision=precision)
            assert states.shape[0] == DT + 1 and sorted(g) == ["b1", "b2", "w1", "w2", "x0"]
            return (states,) + tuple(g[k] for k in sorted(g))
        replayed(ops, fn, S, variants)


# ------------------------------------------------------------------------------------------------------------------ ConditionedNCA
CB, CC, CH, CW = 2, 16, 16, 32       # hidden 64, goal C - 4, alive channel 3


@contextlib.contextmanager
def _force(ops, bits):
    ops.force_generic(bits)
    try:
        yield
    finally:
        ops.force_generic(0)


@contextlib.contextmanager
def _cond_precision(ops, mode):
    ops.set_cond_precision(mode)
    try:
        yield
    finally:
        ops.set_cond_precision(0)


def _cond_variants(B, C, H, W, T, seed, dtype=torch.float32):
    out = []
    for k in range(3):
        x, goal = _inputs(B, C, H, W, seed + 101 * k)
        g = torch.Generator().manual_seed(seed + 101 * k + 50)
        out.append({"x": x.to(dtype), "goal": goal.to(dtype), "u": torch.rand(T, B, 1, H, W, generator=g).to(DEV),
                    "cot": torch.randn(B, C, H, W, generator=g).to(DEV)})
    return out


def _cond_row(ops, T, bits=0, masks="philox", hist=False, dtype=torch.float32, geo=(CB, CC, CH, CW), seed=41, ring=True, **kw):
    """ops.cond_grow: the final state, every ring slot and every pre slot a step writes (ring 2 with T >= 2: all of them; with history:
    states 0 .. T and pre 1 .. T).  ring=False: the final state alone -- all that an eager persistent grow without history defines."""
    B, C, H, W = geo
    assert T >= 2
    variants = _cond_variants(B, C, H, W, T, seed, dtype)
    if masks == "bits":
        for v in variants:
            v["u"] = ops.pack_fire_mask(v["u"], 0.5, "cond")
    S, variants = _statics(variants, ("x", "goal") + (() if masks == "philox" else ("u",)))
    w = _cond_w(ops, _cond_prm(C, seed + 1), S["x"].float())

    def fn():
        with _force(ops, bits):
            out, states, pre = ops.cond_grow(S["x"], T, S["goal"], S.get("u"), w, 3, seed=5 | (3 << 32), step0=1, keep_history=hist)
        return (out, states, pre[1:] if hist else pre) if ring else (out,)
    return fn, replayed(ops, fn, S, variants, **kw)


def _launches(ops, fused, words=None):
    def facts(spy):
        _no_persistent_launch(spy)
        assert ops.fused_step_launches() == fused, (ops.fused_step_launches(), fused)
        assert (ops.fire_word_launches() > 0) if words is None else (ops.fire_word_launches() == words), ops.fire_word_launches()
    return facts


def test_c1_per_step_philox():
    with gpu_ops() as ops:
        _cond_row(ops, 5, bits=_bits(ONE, 1, 0) | NO_FUSED, path_facts=_launches(ops, 0))       # C2's hook word with the off switch


@pytest.mark.parametrize("hist,fw_cap,ms_cap", [(False, ONE, 0), (True, ONE, 0), (False, ONE, 2), (False, 4, 0)])
def test_c2_fused_steps(hist, fw_cap, ms_cap):
    """the fused-steps launch keeps its per-tile step counters and the fire words inside x_final: every replay meets those of other data;
    ms_cap = 2: several fused launches per chunk; fw_cap = 4: chunks 4 + 4 + 1, the counters count on across them"""
    Tn = 9
    want = _expected_launches(Tn, fw_cap, ms_cap, CC)
    assert want == {(ONE, 0): 1, (ONE, 2): 5, (4, 0): 3}[(fw_cap, ms_cap)]
    with gpu_ops() as ops:
        _cond_row(ops, Tn, bits=_bits(fw_cap, 1, ms_cap), hist=hist, seed=43, path_facts=_launches(ops, want))


def test_graph_capture_takes_the_per_step_kernels():
    """C3.  ops.persistent_cond at a covered shape: the capture leaves the persistent grow out (the spy stays empty), and the replay gives
    the bits of the per-step kernels."""
    geo, Tn = (2, 16, 32, 32), 6
    with gpu_ops(persistent_cond=True) as ops:
        assert ops.lib().ncahip_cond_grow_persist_workspace(*geo, 64, 12) > 0
        fn, (refs, last) = _cond_row(ops, Tn, geo=geo, seed=45, ring=False)              # path facts: spy.seen == [] and no epoch asked for
        with _Spy(ops) as spy:
            again = fn()[0].clone()
        assert spy.seen == [(PERSIST_ENTRIES[2], 0)], spy.seen                # the references are the persistent grow's ...
        ops.persistent_cond = False
        with _Spy(ops) as spy:
            ref = fn()[0].clone()                                             # ... and the per-step kernels' on the same inputs (V0)
        assert spy.seen == []
        assert torch.equal(ref, last[0]) and torch.equal(ref, again) and torch.equal(ref, refs[0][0])
        ops.check_errors()


def test_c4_bf16_state_and_goal():
    with gpu_ops() as ops:
        _cond_row(ops, 5, dtype=torch.bfloat16, seed=47)


@pytest.mark.parametrize("masks", ["uniforms", "bits"])
def test_c5_explicit_masks_are_static_inputs(masks):
    with gpu_ops() as ops:
        _cond_row(ops, 5, masks=masks, seed=49, path_facts=_launches(ops, 0, 0))


@pytest.mark.parametrize("geo,dtype", [((2, 16, 16, 16), torch.float32), ((1, 20, 5, 20), torch.float32), ((2, 16, 16, 16), torch.bfloat16)])
def test_c6_history_grow_and_backward_in_one_capture(geo, dtype):
    """(1, 20, 5, 20): the launch_fm<20> class of the backward; bfloat16: the bf16 history and goal.
    These rows found that a replayed graph does not keep a hipMemsetAsync node ahead of the kernel nodes behind it: the driver's three
    accumulators (weight-gradient slabs, wp partials, g_goal) were zeroed under the first step's flush and every replay gave other
    gradients, while the eager call is deterministic.  On a capturing stream the backward drivers now zero them with a kernel."""
    B, C, H, W = geo
    Tn = 3
    with gpu_ops() as ops:
        S, variants = _statics(_cond_variants(B, C, H, W, Tn, 51, dtype), ("x", "goal", "cot"))
        w = _cond_w(ops, _cond_prm(C, 52), S["cot"])

        def fn():
            out, states, pre = ops.cond_grow(S["x"], Tn, S["goal"], None, w, 3, seed=9, step0=4, keep_history=True)
            g = ops.cond_grow_backward(states, pre, S["goal"], None, w, S["cot"], Tn, 3, seed=9, step0=4)
            assert sorted(g) == ["b1", "b2", "goal", "w1", "w2", "w3", "wp", "x0"] and all(t is not None for t in g.values())
            return (out, states, pre[1:]) + tuple(g[k] for k in sorted(g))
        replayed(ops, fn, S, variants)


def test_c7_cond_precision_is_snapshotted_at_enqueue():
    with gpu_ops() as ops:
        _cond_row(ops, 5, seed=53, mode=lambda: _cond_precision(ops, 1), differs_without_mode=True)


# ------------------------------------------------------------------------------------------------------------------ clip drivers
def _bank():
    from oracle import nca_oracle as O
    return torch.tensor([O.SOBEL_X, O.SOBEL_Y, O.LAPLACIAN], dtype=torch.float32).reshape(3, 1, 3, 3).to(DEV)


@pytest.mark.parametrize("out_dtype,out_format", [(torch.float32, "rgb24"), (torch.uint8, "rgb24"), (torch.uint8, "i420")])
def test_v1_clip_cond_then_dynca_clip(out_dtype, out_format):
    """the frame front end and the clip driver in one capture; every tensor the capture touches is on the device beforehand (the filter
    bank included: a host tensor would be uploaded by a synchronous copy).  With ops.persistent_steps on, the eager clips run the
    persistent launches and the captured one asks for no workspace."""
    Fn, B, C, fc, H, W = 2, 1, 12, 96, 16, 16
    with gpu_ops(persistent_steps=True) as ops:
        assert ops.lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, 3) > 0
        variants = []
        for k in range(3):
            g = torch.Generator().manual_seed(61 + 101 * k)
            variants.append({"frames": torch.randint(0, 256, (Fn, B, H, W, 3), generator=g, dtype=torch.uint8).to(DEV),
                             "x": (torch.rand(B, C, H, W, generator=g) - 0.5).to(DEV)})
        S, variants = _statics(variants, ("frames", "x"))
        w, k3 = _dynca_w(ops, C, fc, 3, 62, S["x"]), _bank()

        def fn():
            cond = ops.clip_cond(S["frames"], k3, "mean", True)
            images, state = ops.dynca_clip(S["x"], cond, None, w, 1, 2, 3, DPAD, 0.5, seed=77, step0=5, out_dtype=out_dtype, out_format=out_format)
            return cond, images, state
        replayed(ops, fn, S, variants)
        with _Spy(ops) as spy:
            fn()
        assert spy.epochs == 1                                           # the eager clip does ask for the persistent launches
        ops.check_errors()


def test_v2_dynca_clip_xc():
    Fn, B, C, fc, H, W = 2, 2, 13, 96, 16, 16                           # test_gpu_clip_xc's smallest shape the persistent kernel covers
    with gpu_ops(persistent_steps=True) as ops:
        assert ops.lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, fc, 2) > 0
        variants = []
        for k in range(3):
            g = torch.Generator().manual_seed(63 + 101 * k)
            variants.append({"gray": (torch.rand(Fn, B, H, W, generator=g) * 2 - 1).to(DEV), "cond": (torch.rand(B, 2, H, W, generator=g) * 2 - 1).to(DEV),
                             "x": (torch.rand(B, C, H, W, generator=g) - 0.5).to(DEV)})
        S, variants = _statics(variants, ("gray", "cond", "x"))
        w = _dynca_w(ops, C, fc, 2, 64, S["x"])

        def fn():
            return ops.dynca_clip_xc(S["x"], S["gray"], S["cond"], None, w, 2, 3, 3, DPAD, 0.5, seed=77, step0=5, out_dtype=torch.uint8)
        replayed(ops, fn, S, variants)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_v3_clip_encode_then_cond_clip(dtype):
    Fn, B, C, H, W = 2, 1, 16, 16, 16
    with gpu_ops(persistent_cond=True) as ops:
        assert ops.lib().ncahip_cond_grow_persist_workspace(B, C, H, W, 64, C - 4) > 0
        enc = _encoder(C - 4, 3, 65).to(DEV)
        variants = []
        for k in range(3):
            g = torch.Generator().manual_seed(66 + 101 * k)
            x = torch.rand(B, C, H, W, generator=g) * 0.8
            x[:, 3] = 1.0
            variants.append({"frames": torch.rand(Fn, B, 3, H, W, generator=g).to(DEV), "x": x.to(DEV).to(dtype)})
        S, variants = _statics(variants, ("frames", "x"))
        w = _clip_cond_weights(ops, C, 67, S["frames"])

        def fn():
            goal = ops.clip_encode(S["frames"], enc, dtype)
            images, state = ops.cond_clip(S["x"], goal, None, w, 2, 3, seed=11, step0=5, out_dtype=torch.uint8)
            return goal, images, state
        replayed(ops, fn, S, variants)


def test_v4_clip_resize_yuv420():
    """the first eager call uploads the cached tables; the capture only reads them"""
    N, (H, W), size = 2, (20, 24), (40, 48)                             # a shape of test_gpu_clip_resize
    with gpu_ops() as ops:
        ops.release_workspaces()
        variants = [{"frames": torch.randint(0, 256, (N, 3 * H // 2, W), generator=torch.Generator().manual_seed(68 + k), dtype=torch.uint8).to(DEV)}
                    for k in range(3)]
        S, variants = _statics(variants, ("frames",))

        def fn():
            return (ops.clip_resize_yuv420(S["frames"], size, None, "bicubic", "i420"),)
        replayed(ops, fn, S, variants)
        assert len(ops._RESIZE_TABLES_DEV) == 2
