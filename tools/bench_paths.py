#!/usr/bin/env python3
"""Timings of every path beside bench.py's headline, one JSON line each (median of >= 10 timed iterations after 3 warm-ups;
HIP events on the launch stream).  `python tools/bench_paths.py [names...]`; without names: all.

  cond_train      ConditionedNCA grow with history + backward, B=8 T=16 (fp32 and bf16 history)
  cond_c20        the reference's DEFAULT ConditionedNCA (C = 20, 16 hidden channels): forward, forward with history + fused backward
  cond_small      the reference's default training shape (train.py: C = 20, 64 x 64, batch 8) and C = 16 at that size: launch-bound regime
  cond_small_persist  the persistent ConditionedNCA grow (one launch for the whole grow) against the per-step kernels in the same
                  run: 8 x 20 x 64^2 T = 64 with and without history, 1 x 20 x 256^2 without
  cfg3            BASELINE configs[2] shape: B=32 C=16 256^2 T=96, forward with history + backward, fp32 and bf16
  dynca_fwd       DyNCA forward steps: C=16/fc=128, C=12/fc=96, C=32/fc=128 and C=32/fc=256 at 2x512^2 (configs[4])
  dynca_train     DyNCA forward with history + backward (the C driver): C=16/fc=128, C=12/fc=96, C=32/fc=256 at 2x512^2
  big             working sets beyond the 256 MiB Infinity Cache: perception stencil and fused fp32 step at B=64
  video           B = 1 inference at 256^2 with the shipped video models' shapes, single- and two-scale
  video_clip      a 64-frame clip at 256^2, B = 1, step_n = 8, edge conditioning, Philox masks (C = 12 / fc = 96 and C = 16 / fc = 128,
                  single- and two-scale): the per-frame generator synthesize_video consumed to the end against stylize_clip with
                  float32 frames in / float32 images out and uint8 in / uint8 out; host clock around a device synchronise
  video_clip_xc   the same clip with the ExtraChannels default model (C = 16 / fc = 128 / CPE, two- and single-scale), whose grey frame is
                  the last state channel: (a) the hand loop over forward_nsteps (cat, call, slice) against stylize_clip (b) float32 ->
                  float32 and (c) uint8 -> uint8, the three measured twice over (a b c a b c) so that the spread of (a) is on record
  video_clip_cond the same clip with the reference's default ConditionedNCA (C = 20, E = 16, hidden 64), every frame the goal of its own
                  8 steps: (a) the hand loop over nca.grow + torch.clamp against stylize_clip_conditioned (b) float32 -> float32 and
                  (c) uint8 -> uint8, measured twice over (a b c a b c), with ops.persistent_cond off and on; then the encoder alone,
                  ImageEncoder.forward (front pass + MIOpen) against ops.clip_encode, for 8 frames at 256^2 and 1 frame at 64^2
  steer           steered perception (ops.dynca_direction): in one process, unsteered and under a 'polar' field, B = 1 at 256^2 in one
                  launch (single- and two-scale, fp32 and bf16 MFMA), the 8 x 16 x 256^2 step, and a 64-frame clip through
                  stylize_clip(direction=("polar", 0)) against the same clip without
  trainer_default ConditionedNCATrainer at the reference's own defaults (C = 20, 64 x 64, batch 8, nca_steps [48, 96]): ms per iteration
  loss            the default objective (VGG16 features + batched OT + content + overflow) at 32 x 3 x 256^2, fp32 / bf16 features
  loss_ot         the objective and its OT term alone (precomputed features), ot_impl batched, fused and fused_all alternating in one
                  process: 32 x 3 x 256^2 with bf16 features (configs[2]'s batch) and 8 x 3 x 64^2 (the reference's training shape)
  loss_ot_batched / loss_ot_fused / loss_ot_fused_all   the OT term alone at 32 x 3 x 256^2, one variant, 5 calls: the workload of a
                  kernel trace (not part of a run without names)
  loss_ot_index   the OT term alone (ot_impl fused_all, precomputed features at 32 x 3 x 256^2: layers of 65 536 / 16 384 / 4 096
                  positions sampled, n = 1000) with ot_index_rng numpy and philox alternating in one process (numpy / philox / numpy /
                  philox): host time until the term returns, host clock between two synchronisations around forward + backward, and
                  the three sampler launches' own device time
  loss_slw        the objective with appearance_loss_type 'SlW' and its sliced-Wasserstein term alone (precomputed features, six levels),
                  slw_impl torch and fused alternating in one process: 32 x 3 x 256^2 and 8 x 3 x 64^2, fp32 features
  loss_slw_torch / loss_slw_fused   the sliced-Wasserstein term alone at 32 x 3 x 256^2, one variant, 5 calls: the workload of a kernel
                  trace (not part of a run without names)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]
import torch

import bench
from ncahip import ops

DEV = "cuda"


def timed(fns, iters=10, warm=3):
    """fns: list of callables run back to back per iteration; returns per-callable median ms (events between them)."""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    res = [[] for _ in fns]
    for _ in range(iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
        ev[0].record()
        for i, f in enumerate(fns):
            f()
            ev[i + 1].record()
        torch.cuda.synchronize()
        for i in range(len(fns)):
            res[i].append(ev[i].elapsed_time(ev[i + 1]))
    return [statistics.median(r) for r in res], [min(r) for r in res]


def timed_sync(fns, iters=10, warm=3):
    """As `timed`, but every callable is timed on its own between two device synchronisations, on the host clock: for callables whose
    host part outlasts their device part (the OT term draws its indices on the host) the events of `timed` would credit a callable
    with the overlap of its host part and the device tail of the one before it, which depends on the order they run in."""
    import time
    for _ in range(warm):
        for f in fns:
            f()
    res = [[] for _ in fns]
    for _ in range(iters):
        for i, f in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            res[i].append((time.perf_counter() - t0) * 1e3)
    return [statistics.median(r) for r in res], [min(r) for r in res]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def wide_weights(C, gen, hidden=64):
    """bench.make_weights' distribution at another channel count"""
    return {"perception_net.weight": torch.randn(3 * C, 1, 3, 3, generator=gen) * 0.3,
            "update_net.out.0.weight": torch.randn(hidden, 3 * C, 1, 1, generator=gen) / (3 * C) ** 0.5,
            "update_net.out.0.bias": torch.randn(hidden, generator=gen) * 0.1,
            "update_net.out.2.weight": torch.randn(hidden, hidden, 1, 1, generator=gen) / hidden ** 0.5,
            "update_net.out.2.bias": torch.randn(hidden, generator=gen) * 0.1,
            "update_net.out.4.weight": torch.randn(C, hidden, 1, 1, generator=gen) * (0.02 / hidden ** 0.5)}


def cond_case(B, H=256, W=256, C=16, dtype=torch.float32):
    gen = torch.Generator().manual_seed(0)
    prm = bench.make_weights(gen) if C == 16 else wide_weights(C, gen)
    x = torch.rand(B, C, H, W, generator=gen).to(DEV, dtype)
    goal = (torch.randn(B, C - 4, H, W, generator=gen) * 0.5).to(DEV, dtype)
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    w = ops.CondWeights(prm["perception_net.weight"], prm["update_net.out.0.weight"], prm["update_net.out.0.bias"],
                        prm["update_net.out.2.weight"], prm["update_net.out.2.bias"], prm["update_net.out.4.weight"], x)
    return x, goal, cot, w


def cond_train(B, T, dtype, name, iters=10, C=16, HW=256):
    x, goal, cot, w = cond_case(B, H=HW, W=HW, C=C, dtype=dtype)
    box = {}

    def fwd():
        box["h"] = ops.cond_grow(x, T, goal, None, w, 3, seed=1, step0=0, keep_history=True)

    def bwd():
        _, states, pre = box.pop("h")
        ops.cond_grow_backward(states, pre, goal, None, w, cot, T, 3, seed=1, step0=0)

    (tf, tb), (mf, mb) = timed([fwd, bwd], iters=iters)
    cells = B * HW * HW * T
    flop = 2 * (27 * C + 256 * C + 4096)      # forward flop per cell-update; the backward is ~2.4x that on MFMA
    emit(path=name, C=C, HW=HW, storage=str(dtype).split(".")[-1], B=B, T=T, fwd_frac_f32_mfma=cells * flop / tf / 1e9 / 157.3, fwd_ms=tf, bwd_ms=tb, fwd_us_per_step=tf / T * 1e3,
         bwd_us_per_step=tb / T * 1e3, fwd_bwd_Gcells_s=cells / (tf + tb) / 1e6, bwd_over_fwd=tb / tf,
         history_GB=(T + 1) * x.numel() * x.element_size() / 1e9, min_fwd_ms=mf, min_bwd_ms=mb)


def cond_persist(B, HW, T, hist, C=20):
    """us per step of ops.cond_grow with the persistent grow (ops.persistent_cond) and with the per-step kernels, same inputs"""
    x, goal, _, w = cond_case(B, H=HW, W=HW, C=C)
    default, runs = ops.persistent_cond, {}
    for name, on in (("persistent", True), ("per_step", False)):
        def f(on=on):
            ops.persistent_cond = on
            ops.cond_grow(x, T, goal, None, w, 3, seed=1, step0=0, keep_history=hist)
        runs[name] = timed([f])
    ops.persistent_cond = default
    (tp,), (mp,) = runs["persistent"]
    (ts,), (ms,) = runs["per_step"]
    emit(path="cond_small_persist", C=C, HW=HW, B=B, T=T, history=hist, persistent_us_per_step=tp / T * 1e3,
         per_step_us_per_step=ts / T * 1e3, speedup=ts / tp, min_persistent_us_per_step=mp / T * 1e3, min_per_step_us_per_step=ms / T * 1e3)


def dyn_weights(C, fc, cc, gen):
    k1 = 4 * C + cc
    return ops.DyncaWeights(torch.randn(fc, k1, generator=gen) * (0.5 / k1 ** 0.5), torch.randn(fc, generator=gen) * 0.1,
                            torch.randn(C, fc, generator=gen) * (0.02 / fc ** 0.5), torch.zeros(C), torch.zeros(1, device=DEV))


def dynca(B, C, fc, H, W, T, train, cc=3, pad="circular"):
    gen = torch.Generator().manual_seed(0)
    w = dyn_weights(C, fc, cc, gen)
    x = (torch.rand(B, C, H, W, generator=gen) - 0.5).to(DEV)
    cond = (torch.rand(B, cc, H, W, generator=gen) * 2 - 1).to(DEV)
    cot = torch.randn(B, C, H, W, generator=gen).to(DEV)
    flops = 2 * (27 * C + fc * (5 * C + cc))
    cells = B * H * W * T
    if not train:
        (ms,), (mn,) = timed([lambda: ops.dynca_nsteps(x, T, cond, None, w, pad, 0.5, seed=1)])
        emit(path="dynca_fwd", B=B, C=C, fc=fc, HW=[H, W], T=T, us_per_step=ms / T * 1e3, Gcells_s=cells / ms / 1e6,
             TFLOPs=cells * flops / ms / 1e9, frac_f32_mfma=cells * flops / ms / 1e9 / 157.3, min_us_per_step=mn / T * 1e3)
        return
    box = {}

    def fwd():
        box["h"] = ops.dynca_nsteps(x, T, cond, None, w, pad, 0.5, seed=1, keep_history=True)

    def bwd():
        _, states = box.pop("h")
        ops.dynca_nsteps_backward(states, cond, None, w, cot, None, T, pad, 0.5, seed=1)

    (tf, tb), (mf, mb) = timed([fwd, bwd])
    emit(path="dynca_train", B=B, C=C, fc=fc, HW=[H, W], T=T, fwd_us_per_step=tf / T * 1e3, bwd_us_per_step=tb / T * 1e3,
         fwd_bwd_Gcells_s=cells / (tf + tb) / 1e6, bwd_over_fwd=tb / tf, bwd_TFLOPs=3 * cells * flops / tb / 1e9)


def big():
    # stencil at B=64: 67 MB in + 268 MB out per launch, 3 rotating input/output pairs = 1 GB touched between re-uses
    B, C, H, W = 64, 16, 256, 256
    xs = [torch.randn(B, C, H, W, device=DEV) for _ in range(3)]
    k = [0]

    def st():
        ops.dynca_perceive(xs[k[0] % 3], "replicate")
        k[0] += 1
    (ms,), (mn,) = timed([st], iters=12)
    emit(path="stencil_B64", us=ms * 1e3, TBps=320.0 * B * H * W / ms / 1e9, frac_hbm=320.0 * B * H * W / ms / 1e9 / 8.0, min_us=mn * 1e3,
         working_set_MB=3 * (B * C * H * W * 4 * 5) / 1e6)
    # calibration on the same buffers: what this box's HBM delivers for a write-only stream, for a 1:1 copy and for the stencil's own 1 read :
    # 4 writes shape done by torch's elementwise kernel (a broadcast copy) -- the roof the 8 TB/s figure should be read against
    ys = [torch.empty(B, 4, C, H, W, device=DEV) for _ in range(3)]

    def fill():
        ys[k[0] % 3].fill_(1.0)
        k[0] += 1

    def copy11():
        ys[k[0] % 3].copy_(ys[(k[0] + 1) % 3])
        k[0] += 1

    def bcast():
        ys[k[0] % 3].copy_(xs[k[0] % 3].unsqueeze(1))
        k[0] += 1
    (mf, mc, mb), _ = timed([fill, copy11, bcast], iters=12)
    nb = B * C * H * W * 4
    emit(path="hbm_calibration_B64", fill_TBps=4 * nb / mf / 1e9, copy_TBps=8 * nb / mc / 1e9, read1_write4_TBps=5 * nb / mb / 1e9,
         stencil_over_read1_write4=mb / ms)
    del xs, ys
    x, goal, cot, w = cond_case(B)
    T = 8
    (ms,), (mn,) = timed([lambda: ops.cond_grow(x, T, goal, None, w, 3, seed=1)], iters=10)
    cells = B * H * W * T
    emit(path="cond_fwd_B64", us_per_step=ms / T * 1e3, Gcells_s=cells / ms / 1e6, frac_f32_mfma=cells * 17248 / ms / 1e9 / 157.3,
         state_MB=x.numel() * 4 / 1e6)


def loss_leg():
    """The reference's default objective at BASELINE configs[2]'s batch (32 x 3 x 256^2): VGG16 features (seeded random weights:
    the ImageNet weights cannot be fetched here, the WORK is the same) + OT appearance (batched) + content + overflow, forward and
    backward to the generated images, fp32 and bf16 features."""
    import warnings
    import numpy as np
    from ncahip.loss import Loss
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(256, 256, 3) * 255).astype(np.uint8)
    if os.environ.get("NCAHIP_MIOPEN_BENCHMARK") == "1":      # probe: MIOpen's exhaustive find instead of its immediate-mode pick
        torch.backends.cudnn.benchmark = True
    import time as _time
    _t0 = _time.perf_counter()
    for name, dt, cl in (("float32", torch.float32, False), ("bfloat16", torch.bfloat16, False), ("bfloat16 NHWC", torch.bfloat16, True)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            L = Loss(dev, target_style_image=style, feature_dtype=dt, channels_last=cl)
        gen = torch.rand(32, 3, 256, 256, device=dev, requires_grad=True)
        d = {"generated_images": gen, "nca_state": torch.rand(32, 16, 256, 256, device=dev) * 3 - 1.5,
             "target_images": torch.rand(32, 3, 256, 256, device=dev)}

        def f():
            gen.grad = None
            L(d)[0].backward()
        (ms,), (mn,) = timed([f], iters=10)
        emit(path="cfg3_loss", features=name, B=32, ms_fwd_bwd=ms, min_ms=mn, objective="overflow + OT appearance (batched) + content, VGG16 random weights",
             miopen_benchmark=bool(torch.backends.cudnn.benchmark), wall_s_so_far=_time.perf_counter() - _t0)


OT_IMPLS = ("batched", "fused", "fused_all")


def _ot_fn(impl):
    from ncahip import loss
    return {"batched": loss.ot_loss_batched, "fused": loss.ot_loss_fused, "fused_all": loss.ot_loss_fused_all}[impl]


def _ot_setup(B, S, dt):
    """Loss modules of the three OT variants on one style image, the objective's input dict, and the style / generated features the OT
    term sees (the generated ones detached: leaves of their own, so the OT term's forward + backward can be timed alone)."""
    import warnings
    import numpy as np
    from ncahip.loss import Loss, STYLE_LAYERS
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(S, S, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        L = {impl: Loss(dev, target_style_image=style, feature_dtype=dt, ot_impl=impl) for impl in OT_IMPLS}
    gen = torch.rand(B, 3, S, S, device=dev, requires_grad=True)
    d = {"generated_images": gen, "nca_state": torch.rand(B, 16, S, S, device=dev) * 3 - 1.5, "target_images": torch.rand(B, 3, S, S, device=dev)}
    with torch.no_grad():
        gf = L["batched"].vgg(gen, STYLE_LAYERS)
    tf = [L["batched"].style_feats[l] for l in STYLE_LAYERS]
    gfl = [gf[l].detach().clone().requires_grad_(True) for l in STYLE_LAYERS]
    return L, d, gen, tf, gfl


def loss_ot_leg():
    """ot_impl batched (the torch path) against fused (csrc/nca_ot.hip: relaxed EMD) and fused_all (+ csrc/nca_ot_moment.hip: the
    moment term too), alternating call by call in one process: (a) the whole
    objective, forward + backward to the generated images, (b) the OT term alone on precomputed features, forward + backward to
    the features.  Median of 10 after 3 warm-ups each, host clock between device synchronisations (timed_sync)."""
    import numpy as np
    for B, S, dt, name in ((32, 256, torch.bfloat16, "cfg3 batch, bf16 features"), (8, 64, torch.float32, "reference training shape, fp32 features")):
        L, d, gen, tf, gfl = _ot_setup(B, S, dt)

        def whole(impl):
            def f():
                gen.grad = None
                L[impl](d)[0].backward()
            return f

        def term(fn):
            def f():
                for g in gfl:
                    g.grad = None
                fn(tf, gfl).backward()
            return f
        np.random.seed(0)
        w, wm = timed_sync([whole(impl) for impl in OT_IMPLS], iters=10)
        t, tm = timed_sync([term(_ot_fn(impl)) for impl in OT_IMPLS], iters=10)
        res = {}
        for k, impl in enumerate(OT_IMPLS):
            np.random.seed(1)
            res.update({f"objective_ms_{impl}": w[k], f"objective_min_ms_{impl}": wm[k], f"ot_term_ms_{impl}": t[k],
                        f"ot_term_min_ms_{impl}": tm[k], f"ot_value_{impl}": float(_ot_fn(impl)(tf, gfl))})
        emit(path="loss_ot", shape=f"{B}x3x{S}x{S}", what=name, layers=[list(t.shape[1:]) for t in tf], **res)
        del L, d, gen, tf, gfl
        torch.cuda.empty_cache()


def loss_ot_trace_leg(impl, calls=5):
    """The OT term alone at 32 x 3 x 256^2, forward + backward, `calls` times with one variant and nothing else on the device after
    the features exist: run under a kernel trace, the per-call launch count is (kernel calls after set-up) / calls."""
    import numpy as np
    _, _, _, tf, gfl = _ot_setup(32, 256, torch.bfloat16)
    fn = _ot_fn(impl)
    np.random.seed(0)
    torch.cuda.synchronize()
    emit(path="loss_ot_trace", impl=impl, calls=calls, marker="setup done")
    for _ in range(calls):
        for g in gfl:
            g.grad = None
        fn(tf, gfl).backward()
    torch.cuda.synchronize()


def loss_ot_index_leg():
    """Where the OT term's sampled positions come from: Loss(ot_impl="fused_all") with ot_index_rng "numpy" (np.random.choice per
    (sample, layer) on the host, one upload per layer) against "philox" (ops.ot_sample_idx: one launch per sampled layer), on
    precomputed features of BASELINE configs[2]'s batch.  Four runs in one process, numpy / philox / numpy / philox, so that the
    numpy leg's own run-to-run difference is on record; each the median of 10 after 3 warm-ups of (a) host ms until ot_term returns,
    nothing synchronised, and (b) host ms between two device synchronisations around forward + backward.  Then the three sampler
    launches alone between two events."""
    import time
    import numpy as np
    from ncahip.loss import Loss
    B, S, n = 32, 256, 1000
    _, _, _, tf, gfl = _ot_setup(B, S, torch.bfloat16)
    dev = torch.device(DEV)
    sampled = [t.shape[2] * t.shape[3] for t in tf if t.shape[2] > 32]
    np.random.seed(0)
    for run, rng in enumerate(("numpy", "philox", "numpy", "philox")):
        L = Loss(dev, content_loss_weight=0.0, appearance_loss_weight=0.0, ot_impl="fused_all", ot_index_rng=rng, ot_index_seed=1)
        ret, both = [], []
        for it in range(13):
            for g in gfl:
                g.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = L.ot_term(tf, gfl)
            t1 = time.perf_counter()
            v.backward()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if it >= 3:
                ret.append((t1 - t0) * 1e3)
                both.append((t2 - t0) * 1e3)
        emit(path="loss_ot_index", run=run, ot_index_rng=rng, shape=f"{B}x3x{S}x{S}", sampled_positions=sampled, n=n,
             host_return_ms=statistics.median(ret), host_return_min_ms=min(ret), fwd_bwd_sync_ms=statistics.median(both),
             fwd_bwd_sync_min_ms=min(both), ot_value=float(v.detach()))
    dts = []
    for it in range(13):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for li, hw in enumerate(sampled):
            ops.ot_sample_idx(B, hw, n, 1, (it << 24) | (li << 16), device=dev)
        e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            dts.append(e0.elapsed_time(e1))
    emit(path="loss_ot_index", what="the three sampler launches alone (events around them)", rows=B, sampled_positions=sampled, n=n,
         sampler_device_ms=statistics.median(dts), sampler_device_min_ms=min(dts))


SLW_IMPLS = ("torch", "fused")


def _slw_setup(B, S):
    """Loss modules of the two 'SlW' variants on one style image, the objective's input dict, and the six (source, target) levels the
    term sees: the normalised image and the five style layers, flattened, the generated ones detached leaves of their own."""
    import warnings
    import numpy as np
    from ncahip.loss import Loss, STYLE_LAYERS
    dev = torch.device(DEV)
    style = (np.random.RandomState(0).rand(S, S, 3) * 255).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        L = {impl: Loss(dev, target_style_image=style, appearance_loss_type="SlW", slw_impl=impl) for impl in SLW_IMPLS}
    gen = torch.rand(B, 3, S, S, device=dev, requires_grad=True)
    d = {"generated_images": gen, "nca_state": torch.rand(B, 16, S, S, device=dev) * 3 - 1.5, "target_images": torch.rand(B, 3, S, S, device=dev)}
    Lt = L["torch"]
    flat = lambda f: f.reshape(f.shape[0], f.shape[1], -1)
    norm = lambda im: (im - Lt.vgg.mean) / Lt.vgg.std
    with torch.no_grad():
        gf = Lt.vgg(gen, STYLE_LAYERS)
        src = [flat(norm(gen))] + [flat(gf[l]) for l in STYLE_LAYERS]
        tgt = [flat(norm(Lt.target_style_tensor))] + [flat(Lt.style_feats[l]) for l in STYLE_LAYERS]
    src = [x.detach().clone().requires_grad_(True) for x in src]
    return L, d, gen, src, tgt


def _slw_term(impl, src, tgt):
    from ncahip import loss
    fn = loss._SLW_IMPLS[impl]

    def f():
        for x in src:
            x.grad = None
        total = sum(fn(x, y) for x, y in zip(src, tgt))
        total.backward()
        return total
    return f


def loss_slw_leg():
    """slw_impl torch (einsum, torch.sort, autograd) against fused (csrc/nca_slw.hip), alternating call by call in one process: (a) the
    whole objective with appearance_loss_type 'SlW', forward + backward to the generated images, (b) the sliced-Wasserstein term
    alone on precomputed features (six levels), forward + backward to the features.  Median of 10 after 3 warm-ups each, host clock
    between device synchronisations (timed_sync).  Both variants draw their projections from torch's CPU generator, seeded alike."""
    for B, S, name in ((32, 256, "cfg3 batch, fp32 features"), (8, 64, "reference training shape, fp32 features")):
        L, d, gen, src, tgt = _slw_setup(B, S)

        def whole(impl):
            def f():
                gen.grad = None
                L[impl](d)[0].backward()
            return f
        torch.manual_seed(0)
        w, wm = timed_sync([whole(impl) for impl in SLW_IMPLS], iters=10)
        t, tm = timed_sync([_slw_term(impl, src, tgt) for impl in SLW_IMPLS], iters=10)
        res = {}
        for k, impl in enumerate(SLW_IMPLS):
            torch.manual_seed(1)
            res.update({f"objective_ms_{impl}": w[k], f"objective_min_ms_{impl}": wm[k], f"slw_term_ms_{impl}": t[k],
                        f"slw_term_min_ms_{impl}": tm[k], f"slw_value_{impl}": float(_slw_term(impl, src, tgt)())})
        ops.check_errors()
        emit(path="loss_slw", shape=f"{B}x3x{S}x{S}", what=name, levels=[[x.shape[1], x.shape[2], y.shape[2]] for x, y in zip(src, tgt)], **res)
        del L, d, gen, src, tgt
        torch.cuda.empty_cache()


def loss_slw_trace_leg(impl, calls=5):
    """The sliced-Wasserstein term alone at 32 x 3 x 256^2, forward + backward, `calls` times with one variant and nothing else on the
    device after the features exist: run under a kernel trace, the per-call launch count is (kernel calls after set-up) / calls."""
    _, _, _, src, tgt = _slw_setup(32, 256)
    f = _slw_term(impl, src, tgt)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    emit(path="loss_slw_trace", impl=impl, calls=calls, marker="setup done")
    for _ in range(calls):
        f()
    torch.cuda.synchronize()


def trainer_default_leg():
    """ConditionedNCATrainer at the reference's OWN defaults (EncoderConditioning/train.py:30-50: default ConditionedNCA = C 20, 64 x 64
    targets, batch 8, nca_steps [48, 96] drawn per batch, pool 512, lr 2e-3): wall time per trainer iteration (two train_batch calls:
    grow with history, objective, fused backward, per-tensor normalisation, Adam, pool write-back) with the default objective (OT +
    content + overflow on seeded-random VGG16 features) and with a stand-in objective, fp32 and bf16 pool; host overhead included."""
    import tempfile, time, warnings
    import numpy as np
    from ncahip.conditioned_trainer import ConditionedNCATrainer, PhaseTimer
    from ncahip.loss import Loss
    from ncahip.nca import ConditionedNCA
    dev = torch.device(DEV)
    S = 64

    class Targets:
        target_size = (3, S, S)

        def __init__(self):
            self.data = torch.rand(16, 3, S, S, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

        def __len__(self):
            return self.data.shape[0]

        def __getitem__(self, idx):
            return self.data[torch.as_tensor(idx, device=dev)]

    class StandIn(torch.nn.Module):
        def forward(self, d):
            s = d["nca_state"].float()
            return [(d["generated_images"].float() - d["target_images"]).square().mean() + (s - s.clamp(-1.0, 1.0)).abs().mean(), {}]

    style = (np.random.RandomState(0).rand(S, S, 3) * 255).astype(np.uint8)
    for name, dt, default_obj in (("default objective", torch.float32, True), ("stand-in objective", torch.float32, False),
                                  ("stand-in objective", torch.bfloat16, False)):
        torch.manual_seed(0)
        nca = ConditionedNCA(target_shape=(3, S, S)).to(dev)          # the reference's default arguments: C = 20
        if default_obj:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                objective = Loss(dev, target_style_image=style, feature_dtype=torch.bfloat16)
        else:
            objective = StandIn()
        tr = ConditionedNCATrainer(nca, Targets(), None, nca_steps=[48, 96], pool_size=512, loss=objective, device=dev,
                                   log_base_path=tempfile.mkdtemp(prefix="ncahip_bench_"), pool_dtype=dt)
        for i in range(3):
            tr._iteration(i, 8)
        torch.cuda.synchronize()
        tr.phase_timer = PhaseTimer()
        times, steps, phases = [], [], []
        for i in range(12):
            tr.phase_timer.reset()
            s0 = nca._mask_step
            t0 = time.perf_counter()
            tr._iteration(3 + i, 8)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            steps.append(nca._mask_step - s0)
            phases.append(tr.phase_timer.summary())
        med = statistics.median(times)
        per_step = statistics.median([t / max(1, n) for t, n in zip(times, steps)])
        ph = {k: round(float(np.median([p.get(k, 0.0) for p in phases])), 3) for k in sorted({k for p in phases for k in p})}
        emit(path="trainer_default", objective=name, pool=str(dt).split(".")[-1], C=nca.num_channels, HW=S, batch=8, ms_per_iteration=med * 1e3,
             nca_steps_per_iteration_median=statistics.median(steps), wall_us_per_nca_step=per_step * 1e6, phase_ms_per_iteration=ph)
        tr.phase_timer = None
        del tr, objective


def video_leg():
    """B = 1 inference as the video loop issues it (utils/misc/video_utils.py:66-83: forward_nsteps(h, step_n, cond_img=frame) per
    frame) with the shipped video models' shapes (C = 12 / fc = 96 and C = 16 / fc = 128, pos_emb, two-scale perception), 256^2."""
    for C, fc in ((12, 96), (16, 128)):
        for two in (False, True):
            gen = torch.Generator().manual_seed(0)
            w = dyn_weights(C, fc, 2, gen)
            x = (torch.rand(1, C, 256, 256, generator=gen) - 0.5).to(DEV)
            cond = (torch.rand(1, 2, 256, 256, generator=gen) * 2 - 1).to(DEV)
            T = int(os.environ.get("NCAHIP_VIDEO_T", "32"))      # steps per frame (one forward_nsteps call)
            res = {}
            for persist in (True, False):     # the one-launch persistent kernel vs one launch per step
                ops.persistent_steps = persist
                (ms,), (mn,) = timed([lambda: ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, two_scale=two)], iters=20)
                res["persistent" if persist else "per_step"] = (ms, mn)
            ops.persistent_steps = True
            ops.check_errors()
            ms, mn = res.get("persistent", res["per_step"])
            flops = 2 * (27 * C + fc * (5 * C + 2))
            emit(path="video_B1", C=C, fc=fc, two_scale=two, HW=[256, 256], us_per_step=ms / T * 1e3, min_us_per_step=mn / T * 1e3,
                 steps_per_call=T, frames_per_s_at_32_steps=1e3 / (ms * 32 / T), kernel="persistent (one launch for T steps)" if "persistent" in res else "per-step launches",
                 per_step_launch_us_per_step=res["per_step"][0] / T * 1e3, frac_f32_mfma=256 * 256 * T * flops / ms / 1e9 / 157.3)


def video_clip_leg():
    """What a user does with a trained model: a clip in, a stylised clip out (utils/misc/video_utils.py:50-83).  (a) the Python
    generator ncahip.video.synthesize_video, one frame at a time; (b) ncahip.video.stylize_clip, float32 [F,3,H,W] in, float32 out;
    (c) stylize_clip, uint8 [F,H,W,3] in, uint8 out.  Frames live on the device; every call seeds the state anew, so each timed call
    does the same work.  The host part of (a) outlasts its device part, so each call is timed on the host clock between two device
    synchronisations (timed_sync): median of 10 after 3 warm-ups."""
    from ncahip import video
    from ncahip.models.dynca import DyNCA
    n_frames, step_n, S = 64, 8, 256
    for C, fc in ((12, 96), (16, 128)):
        for two in (False, True):
            torch.manual_seed(0)
            m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning="edges", edge_transform="tanh",
                      perception_scales=[0, 1] if two else [0], device=torch.device(DEV))
            m.mask_rng, m.mask_seed = "philox", 1
            gen = torch.Generator().manual_seed(0)
            u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=gen, dtype=torch.uint8).to(DEV)
            f32 = (u8.float() / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()
            frame_list = list(f32)

            def loop():
                for _ in video.synthesize_video(m, frame_list, step_n=step_n):
                    pass

            fns, names = [loop], ["synthesize_video"]
            if hasattr(video, "stylize_clip"):
                fns += [lambda: video.stylize_clip(m, f32, step_n=step_n), lambda: video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8)]
                names += ["stylize_clip_f32", "stylize_clip_u8"]
            med, mn = timed_sync(fns)
            ops.check_errors()
            res = {n: dict(us_per_frame=a / n_frames * 1e3, min_us_per_frame=b / n_frames * 1e3, frames_per_s=n_frames / a * 1e3)
                   for n, a, b in zip(names, med, mn)}
            ratios = {n + "_over_synthesize_video": res[n]["us_per_frame"] / res["synthesize_video"]["us_per_frame"] for n in names[1:]}
            emit(path="video_clip", C=C, fc=fc, two_scale=two, HW=[S, S], frames=n_frames, step_n=step_n, masks="philox",
                 route=getattr(getattr(video, "stylize_clip", None), "last_path", None), **res, **ratios)


def steer_leg():
    """What a direction field costs: every row times the same call unsteered and under steer.direction_field('polar', 0), alternating in
    one process (plain, steered per iteration).  B = 1 at 256^2: video_leg's shape (pos_emb conditioning, T = 32 in one launch)."""
    from ncahip import steer, video
    from ncahip.models.dynca import DyNCA
    T = 32
    for C, fc in ((12, 96), (16, 128)):
        for two in (False, True):
            for precision in ("f32", "bf16"):
                gen = torch.Generator().manual_seed(0)
                w = dyn_weights(C, fc, 2, gen)
                x = (torch.rand(1, C, 256, 256, generator=gen) - 0.5).to(DEV)
                cond = (torch.rand(1, 2, 256, 256, generator=gen) * 2 - 1).to(DEV)
                dirs = steer.direction_field("polar", 0.0, 256, 256, DEV)
                run = lambda: ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1, two_scale=two)      # noqa: E731

                def steered():
                    with ops.dynca_direction(dirs):
                        return run()

                with ops.dynca_precision(precision):
                    assert run()[1] is None and steered()[1] is None          # both took the one-launch kernel
                    (a, b), (amin, bmin) = timed([run, steered], iters=20)
                ops.check_errors()
                emit(path="steer_video_B1", C=C, fc=fc, two_scale=two, precision=precision, HW=[256, 256], steps_per_call=T,
                     us_per_step=a / T * 1e3, steered_us_per_step=b / T * 1e3, min_us_per_step=amin / T * 1e3,
                     min_steered_us_per_step=bmin / T * 1e3, steered_over_plain=b / a)
    for B, C, fc in ((8, 16, 128), (8, 12, 96)):
        gen = torch.Generator().manual_seed(0)
        w = dyn_weights(C, fc, 3, gen)
        x = (torch.rand(B, C, 256, 256, generator=gen) - 0.5).to(DEV)
        cond = (torch.rand(B, 3, 256, 256, generator=gen) * 2 - 1).to(DEV)
        dirs = steer.direction_field("polar", 0.0, 256, 256, DEV)
        run = lambda: ops.dynca_nsteps(x, T, cond, None, w, "circular", 0.5, seed=1)      # noqa: E731

        def steered():
            with ops.dynca_direction(dirs):
                return run()

        (a, b), (amin, bmin) = timed([run, steered])
        emit(path="steer_dynca_fwd", B=B, C=C, fc=fc, HW=[256, 256], T=T, us_per_step=a / T * 1e3, steered_us_per_step=b / T * 1e3,
             min_us_per_step=amin / T * 1e3, min_steered_us_per_step=bmin / T * 1e3, steered_over_plain=b / a)
    n_frames, step_n, S = 64, 8, 256
    for C, fc, two in ((12, 96, False), (16, 128, True)):
        torch.manual_seed(0)
        m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", conditioning="edges", edge_transform="tanh",
                  perception_scales=[0, 1] if two else [0], device=torch.device(DEV))
        m.mask_rng, m.mask_seed = "philox", 1
        u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
        fns = [lambda: video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8),
               lambda: video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8, direction=("polar", 0.0))]
        (a, b), (amin, bmin) = timed_sync(fns)
        ops.check_errors()
        emit(path="steer_video_clip", C=C, fc=fc, two_scale=two, HW=[S, S], frames=n_frames, step_n=step_n, masks="philox", route=video.stylize_clip.last_path,
             us_per_frame=a / n_frames * 1e3, steered_us_per_frame=b / n_frames * 1e3, min_us_per_frame=amin / n_frames * 1e3,
             min_steered_us_per_frame=bmin / n_frames * 1e3, steered_over_plain=b / a)


def video_clip_xc_leg():
    """video_clip_leg for the extra-channel family (ExtraChannels/utils/misc/video_utils.py:66-82; fit_video_motion.py's default model).
    (a) the reference's loop by hand: per frame h = cat(h, mean grey), forward_nsteps, h = state[:, :-1], one image; (b) stylize_clip
    float32 in / float32 out; (c) uint8 in / uint8 out.  Frames on the device, every call seeds anew, host clock between two device
    synchronisations, median of 10 after 3 warm-ups; two passes over (a, b, c): the two (a) figures give the session's spread."""
    from ncahip import video
    from ncahip.models.dynca_extra import DyNCA
    n_frames, step_n, S, C, fc = 64, 8, 256, 16, 128
    for two in (True, False):
        torch.manual_seed(0)
        m = DyNCA(C, 3, fc_dim=fc, padding_mode="circular", pos_emb="CPE", perception_scales=[0, 1] if two else [0], device=torch.device(DEV))
        m.mask_rng, m.mask_seed = "philox", 1
        gen = torch.Generator().manual_seed(0)
        u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=gen, dtype=torch.uint8).to(DEV)
        f32 = (u8.float() / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()

        @torch.no_grad()
        def loop():
            h = m.seed(1, size=(S, S))
            for f in range(n_frames):
                state, rgb = m.forward_nsteps(torch.cat((h, f32[f:f + 1].mean(1, keepdim=True)), 1), step_n)
                h = state[:, :-1]
                (rgb.clamp(-1.0, 1.0) + 1.0) / 2.0

        fns = [loop, lambda: video.stylize_clip(m, f32, step_n=step_n), lambda: video.stylize_clip(m, u8, step_n=step_n, out_dtype=torch.uint8)]
        names = ["hand_loop", "stylize_clip_f32", "stylize_clip_u8"]
        for run in (1, 2):
            med, mn = timed_sync(fns)
            ops.check_errors()
            res = {n: dict(us_per_frame=a / n_frames * 1e3, min_us_per_frame=b / n_frames * 1e3, frames_per_s=n_frames / a * 1e3)
                   for n, a, b in zip(names, med, mn)}
            ratios = {n + "_over_hand_loop": res[n]["us_per_frame"] / res["hand_loop"]["us_per_frame"] for n in names[1:]}
            emit(path="video_clip_xc", run=run, C=C, fc=fc, two_scale=two, HW=[S, S], frames=n_frames, step_n=step_n, masks="philox",
                 route=video.stylize_clip.last_path, **res, **ratios)


def video_clip_cond_leg():
    """video_clip_leg for ConditionedNCA (EncoderConditioning/visualisation.ipynb: the goal switched while the state runs).  (a) the loop by
    hand: per frame state = nca.grow(state, step_n, frame[None]), clamp(state[:, :3], 0, 1); (b) stylize_clip_conditioned float32 in /
    float32 out; (c) uint8 in / uint8 out.  Frames on the device, a dense state (alive everywhere) so that every step does real work, host
    clock between two device synchronisations, median of 10 after 3 warm-ups; two passes over (a, b, c): the two (a) figures give the
    session's spread.  At 256^2 the persistent grow needs all 256 CUs: a poll that expires is reported, not retried."""
    from ncahip import video
    from ncahip.nca import ConditionedNCA
    n_frames, step_n, S = 64, 8, 256
    torch.manual_seed(0)
    m = ConditionedNCA(target_shape=(3, S, S)).to(DEV)
    with torch.no_grad():
        m.update_net.out[4].weight.mul_(0.3)
    m.mask_rng, m.mask_seed = "philox", 1
    gen = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (n_frames, S, S, 3), generator=gen, dtype=torch.uint8).to(DEV)
    f32 = (u8.float() / 255.0).permute(0, 3, 1, 2).contiguous()
    x0 = torch.rand(1, m.num_channels, S, S, generator=gen) * 0.5
    x0[:, 3] = 1.0
    x0 = x0.to(DEV)

    @torch.no_grad()
    def loop():
        state = x0
        for f in range(n_frames):
            state = m.grow(state, step_n, f32[f:f + 1])
            torch.clamp(state[:, :3], 0.0, 1.0)

    fns = [loop, lambda: video.stylize_clip_conditioned(m, f32, step_n=step_n, state=x0),
           lambda: video.stylize_clip_conditioned(m, u8, step_n=step_n, state=x0, out_dtype=torch.uint8)]
    names = ["hand_loop", "stylize_clip_conditioned_f32", "stylize_clip_conditioned_u8"]
    keep = ops.persistent_cond
    try:
        for persistent in (False, True):
            ops.persistent_cond = persistent
            if persistent:      # one grow first: if its polls expire here, the clip legs (64 launches each) are not started
                try:
                    with torch.no_grad():
                        m.grow(x0, step_n, f32[:1])
                    ops.check_errors()
                except Exception as e:
                    emit(path="video_clip_cond", persistent_cond=True, error="probe grow: " + str(e)[:300])
                    break
            for run in (1, 2):
                try:
                    med, mn = timed_sync(fns)
                    ops.check_errors()
                except Exception as e:      # a bounded poll of the persistent grow expired (another process holds CUs): on record, no retry
                    emit(path="video_clip_cond", run=run, persistent_cond=persistent, error=str(e)[:300])
                    try:
                        ops.check_errors()
                    except Exception:
                        pass
                    break
                res = {n: dict(us_per_frame=a / n_frames * 1e3, min_us_per_frame=b / n_frames * 1e3, frames_per_s=n_frames / a * 1e3)
                       for n, a, b in zip(names, med, mn)}
                ratios = {n + "_over_hand_loop": res[n]["us_per_frame"] / res["hand_loop"]["us_per_frame"] for n in names[1:]}
                emit(path="video_clip_cond", run=run, persistent_cond=persistent, C=m.num_channels, E=m.num_hidden_channels, HW=[S, S],
                     frames=n_frames, step_n=step_n, masks="philox", route=video.stylize_clip_conditioned.last_path, **res, **ratios)
    finally:
        ops.persistent_cond = keep
    # the encoder alone: the module's forward (HIP front pass, two MIOpen convolutions, bias, ReLU) against the one fused launch
    for n, s in ((8, 256), (1, 64)):
        fr = f32[:n, :, :s, :s].contiguous()
        with torch.no_grad():
            enc_fns = [lambda: m.encoder(fr), lambda: ops.clip_encode(fr.unsqueeze(1), m.encoder)]
            for run in (1, 2):
                med, mn = timed_sync(enc_fns)
                emit(path="video_clip_cond_encoder", run=run, frames=n, HW=[s, s], E=m.num_hidden_channels,
                     module_forward_us=med[0] * 1e3, module_forward_min_us=mn[0] * 1e3, clip_encode_us=med[1] * 1e3, clip_encode_min_us=mn[1] * 1e3,
                     clip_encode_over_module=med[1] / med[0])
    ops.check_errors()


def main(names):
    allp = not names
    if allp or "cond_train" in names:
        cond_train(8, 16, torch.float32, "cond_train")
        cond_train(8, 16, torch.bfloat16, "cond_train")
    if allp or "cond_c20" in names:
        cond_train(8, 16, torch.float32, "cond_c20", C=20)
        cond_train(8, 16, torch.bfloat16, "cond_c20", C=20)     # bf16 pool: bf16-MFMA forward, bf16 history, exact-f32 products in the backward
        cond_train(8, 16, torch.float32, "cond_c32", C=32)
    if allp or "cond_small" in names:
        # the reference's own DEFAULT training shape (EncoderConditioning/train.py:36-43: 16 hidden channels -> C = 20, 64 x 64, batch 8)
        cond_train(8, 64, torch.float32, "cond_small_default", C=20, HW=64)
        cond_train(8, 64, torch.float32, "cond_small", C=16, HW=64)
        cond_train(8, 64, torch.bfloat16, "cond_small", C=16, HW=64)
    if allp or "cond_small_persist" in names:
        cond_persist(8, 64, 64, True)      # the training forward (history for the backward)
        cond_persist(8, 64, 64, False)
        cond_persist(1, 256, 64, False)
    if allp or "cfg3" in names:
        cond_train(32, 96, torch.float32, "cfg3", iters=10)
        cond_train(32, 96, torch.bfloat16, "cfg3", iters=10)
    if allp or "dynca_fwd" in names:
        dynca(8, 16, 128, 256, 256, 32, False)
        dynca(8, 12, 96, 256, 256, 32, False)
        dynca(2, 32, 128, 512, 512, 16, False)
        dynca(2, 32, 256, 512, 512, 16, False)
    if allp or "dynca_train" in names:
        dynca(8, 16, 128, 256, 256, 16, True)
        dynca(8, 12, 96, 256, 256, 16, True)
        dynca(2, 32, 256, 512, 512, 8, True)
    if allp or "big" in names:
        big()
    if allp or "loss" in names:
        loss_leg()
    if allp or "loss_ot" in names:
        loss_ot_leg()
    for impl in OT_IMPLS:
        if "loss_ot_" + impl in names:
            loss_ot_trace_leg(impl)
    if allp or "loss_ot_index" in names:
        loss_ot_index_leg()
    if allp or "loss_slw" in names:
        loss_slw_leg()
    for impl in SLW_IMPLS:
        if "loss_slw_" + impl in names:
            loss_slw_trace_leg(impl)
    if allp or "video" in names:
        video_leg()
    if allp or "video_clip" in names:
        video_clip_leg()
    if allp or "video_clip_xc" in names:
        video_clip_xc_leg()
    if allp or "video_clip_cond" in names:
        video_clip_cond_leg()
    if allp or "steer" in names:
        steer_leg()
    if allp or "trainer_default" in names:
        trainer_default_leg()


if __name__ == "__main__":
    main(sys.argv[1:])
