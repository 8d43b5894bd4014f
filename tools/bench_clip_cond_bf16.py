#!/usr/bin/env python3
"""Time stylize_clip_conditioned on a bf16 state (ncahip_clip_encode_bf16, ncahip_cond_clip_bf16 and its fused finalize + image launch)
against the fp32 clip route and against what a bf16 caller got before, and write profiles/clip_cond_bf16.jsonl.

    python tools/bench_clip_cond_bf16.py --other-lib PATH/libncahip.so [--out profiles/clip_cond_bf16.jsonl]

One job: this process never touches the GPU.  Every GPU step is a child process of its own under `timeout`, one after the other, and
the first that fails ends the job (what `a && b && c` does in a shell).  The steps:

  parent / this, run 1 and 2   stylize_clip_conditioned as it is called without the precision keyword, on the library of the parent
   (order: parent, this,       commit (--other-lib) and on this tree's: a bf16 state (the Python loop over nca.grow: what a bf16 caller
    this, parent)              got so far) and an fp32 state (the clip route).  This tree's fp32 clip has to lie inside the spread of
                               the parent's two runs -- the old path is undisturbed; the job's only pass / fail figure.
  bf16, run 1 and 2            this tree, precision='bf16': float32, uint8 and I420 images.
  kernels                      the fused encoder alone at 8 x 256^2, fp32 goal against bf16 goal; ncahip_cond_finalize_emit_bf16 against
                               ncahip_cond_finalize_bf16 + ncahip_clip_emit_unit_bf16 at 1 x 20 x 256^2 (float32, uint8, I420 images):
                               50 launches queued behind a busy stream, device events around them, median of 10 samples.

Setup of the stylize legs: the default model (C = 20, E = 16, hidden 64), 64 float32 frames of 256 x 256 on the device, step_n = 8,
Philox masks, a dense state (alive everywhere), frames_per_call = 8.  Host clock between two synchronisations, median of 10 after 3
warm-ups."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]

DEV = "cuda"
S, BATCH = 256, 50
F, STEP_N = 64, 8
STEP_LIMIT = 240        # seconds per GPU step


def timed_queued(torch, fn, busy, iters=10, warm=2):
    """median and minimum microseconds per call of fn, BATCH calls queued behind a busy stream, device events around them"""
    ts = []
    for i in range(warm + iters):
        for _ in range(6):
            busy @ busy
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BATCH):
            fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b) / BATCH * 1e3)
    return statistics.median(ts), min(ts)


def timed_sync(torch, fn, iters=10, warm=3):
    """median and minimum ms of fn on the host clock between two device synchronisations"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def setup(torch):
    from ncahip.nca import ConditionedNCA
    torch.manual_seed(0)
    m = ConditionedNCA(target_shape=(3, S, S))                      # the default model: C = 3 + 1 + 16, E = 16, hidden 64
    with torch.no_grad():
        m.update_net.out[4].weight.mul_(0.3)
    m = m.to(DEV)
    m.mask_rng, m.mask_seed = "philox", 1
    gen = torch.Generator().manual_seed(2)
    frames = torch.rand(F, 3, S, S, generator=gen).to(DEV)
    x0 = torch.rand(1, 20, S, S, generator=gen) * 0.8
    x0[:, 3] = 1.0
    return m, frames, x0.to(DEV)


def stylize_step(emit, label, run, bf16_keyword):
    """one GPU step of the stylize legs"""
    import torch
    from ncahip import _capi, ops, video
    if label == "parent":                                  # an older library lacks the newer exports: bind what it has
        import ctypes
        probe = ctypes.CDLL(_capi.LIB_PATH)
        for name in [n for n in _capi.SIGNATURES if not hasattr(probe, n)]:
            del _capi.SIGNATURES[name]
    ops.selftest()
    m, frames, x0 = setup(torch)

    def leg(name, want_path, state, **kw):
        def call():
            m._mask_step = 0
            return video.stylize_clip_conditioned(m, frames, step_n=STEP_N, state=state, **kw)
        med, mn = timed_sync(torch, call)
        assert video.stylize_clip_conditioned.last_path == want_path, (name, video.stylize_clip_conditioned.last_path)
        emit(leg="stylize", route=name, library="parent" if label == "parent" else "this", run=run, frames=F, step_n=STEP_N, size=[S, S],
             us_per_frame=med / F * 1e3, min_us_per_frame=mn / F * 1e3)

    if bf16_keyword:
        leg("bf16 clip, float32 images", "clip", x0, precision="bf16")
        leg("bf16 clip, uint8 images", "clip", x0, precision="bf16", out_dtype=torch.uint8)
        leg("bf16 clip, i420 images", "clip", x0, precision="bf16", out_dtype=torch.uint8, out_format="i420")
    else:
        leg("bf16 state, no keyword (loop)", "loop", x0.to(torch.bfloat16))
        leg("fp32 clip", "clip", x0)
    ops.check_errors()


def kernels_step(emit):
    import torch
    from ncahip import _capi, ops
    ops.selftest()
    L, st = ops.lib(), ops._stream()
    BF = torch.bfloat16
    busy = torch.randn(4096, 4096, device=DEV)
    m, frames, x0 = setup(torch)
    # the encoder alone: one chunk of 8 frames
    chunk = frames[:8].unsqueeze(1).contiguous()
    enc = m.encoder
    k3 = ops._w(torch.cat((enc.sobel_x.weight, enc.sobel_y.weight, enc.laplacian.weight), dim=0).reshape(-1), "k3", chunk)
    k5 = ops._w(enc.gaussian_blur.weight.reshape(-1), "k5", chunk)
    w1, b1, w2 = (ops._w(t, "w", chunk) for t in (enc.embed[0].weight, enc.embed[0].bias, enc.embed[2].weight))
    for dtype, name in ((torch.float32, "fp32 goal"), (BF, "bf16 goal")):
        goal = torch.empty(8, 1, 16, S, S, device=DEV, dtype=dtype)
        fn = L.ncahip_clip_encode if dtype == torch.float32 else L.ncahip_clip_encode_bf16

        def encode(fn=fn, goal=goal):                      # the C call alone on preallocated buffers
            return fn(chunk.data_ptr(), _capi.CLIP_F32_NCHW, k3.data_ptr(), k5.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), goal.data_ptr(),
                      8, 1, 3, 16, S, S, st)

        assert encode() == 0 and torch.equal(goal, ops.clip_encode(chunk, enc).to(dtype))                                     # what is timed is right
        for run in (1, 2):
            med, mn = timed_queued(torch, encode, busy)
            emit(leg="encoder", goal=name, run=run, shape=[8, 1, 3, S, S], E=16, us_per_launch=med, min_us_per_launch=mn, us_per_frame=med / 8)
    # finalize + image: one launch against two, on a real pending state
    goal = ops.clip_encode(chunk[:1], m.encoder, dtype=BF)[0]
    x_pend, pre = ops.cond_step(x0.to(BF), None, goal, None, m._weights(x0), seed=1, step=0)
    x_out, x_two = torch.empty_like(x_pend), torch.empty_like(x_pend)
    for out_dtype, out_format in ((torch.float32, "rgb24"), (torch.uint8, "rgb24"), (torch.uint8, "i420")):
        spec = ops.ImageSpec.of(out_dtype, out_format, "bt709", "limited", 3, S, S)
        img, img_two = spec.images(1, 1, DEV)[0], spec.images(1, 1, DEV)[0]
        args = (1, 20, S, S, 3, 0.1, -10.0, 10.0, st)

        def fused():
            return L.ncahip_cond_finalize_emit_bf16(x_pend.data_ptr(), pre.data_ptr(), x_out.data_ptr(), img.data_ptr(), spec.fmt, *args)

        def two():
            rc = L.ncahip_cond_finalize_bf16(x_pend.data_ptr(), pre.data_ptr(), x_two.data_ptr(), *args)
            return rc or L.ncahip_clip_emit_unit_bf16(x_two.data_ptr(), img_two.data_ptr(), spec.fmt, 1, 20, S, S, st)

        assert fused() == 0 and two() == 0
        assert torch.equal(x_out, x_two) and torch.equal(img, img_two) and int((img != 0).sum()) > 0                         # what is timed is right
        name = f"{'float32' if out_dtype == torch.float32 else 'uint8'} {out_format}"
        for run in (1, 2):
            for what, fn, n in (("finalize + image, one launch", fused, 1), ("finalize, then image", two, 2)):
                med, mn = timed_queued(torch, fn, busy)
                emit(leg="finalize_emit", image=name, what=what, launches=n, run=run, shape=[1, 20, S, S], us_per_image=med, min_us_per_image=mn)
    ops.check_errors()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_cond_bf16.jsonl"))
    ap.add_argument("--other-lib", default=None, help="the libncahip.so built from the parent commit")
    ap.add_argument("--step", default=None, help="(a child's mode) parent | this | bf16 | kernels: run that GPU step and print its rows")
    ap.add_argument("--run", type=int, default=1)
    args = ap.parse_args()

    def show(**kw):
        print(json.dumps(kw), flush=True)

    if args.step:
        if args.step == "kernels":
            kernels_step(show)
        else:
            stylize_step(show, args.step, args.run, args.step == "bf16")
        return

    if not args.other_lib or not os.path.exists(args.other_lib):
        sys.exit("bench_clip_cond_bf16: --other-lib PATH/libncahip.so (a build of the parent commit) is required")
    lines = []
    steps = [("parent", 1), ("this", 1), ("this", 2), ("parent", 2), ("bf16", 1), ("bf16", 2), ("kernels", 1)]      # neither library always second
    for step, run in steps:                              # one after the other; the first failure ends the job
        env = dict(os.environ, NCAHIP_LIB=os.path.abspath(args.other_lib)) if step == "parent" else dict(os.environ)
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--step", step, "--run", str(run)]
        done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
        for line in done.stdout.splitlines():
            if line.startswith("{"):
                print(line, flush=True)
                lines.append(json.loads(line))
        if done.returncode != 0:
            sys.exit(f"bench_clip_cond_bf16: step {step} (run {run}) ended with status {done.returncode}; nothing more is started")

    def figs(route, library):
        return [r["us_per_frame"] for r in lines if r.get("leg") == "stylize" and r["route"] == route and r["library"] == library]

    parent, this = figs("fp32 clip", "parent"), figs("fp32 clip", "this")
    loop = statistics.mean(figs("bf16 state, no keyword (loop)", "parent"))
    inside = min(parent) <= statistics.mean(this) <= max(parent)
    summary = {"leg": "summary", "fp32_clip_parent_us_per_frame": parent, "fp32_clip_this_us_per_frame": this,
               "fp32_clip_this_inside_parent_spread": inside, "bf16_loop_parent_us_per_frame": loop}
    for name in ("float32", "uint8", "i420"):
        c = statistics.mean(figs(f"bf16 clip, {name} images", "this"))
        summary[f"bf16_clip_{name}_us_per_frame"] = c
        summary[f"bf16_clip_{name}_over_bf16_loop"] = c / loop
        summary[f"bf16_clip_{name}_over_fp32_clip"] = c / statistics.mean(this)
    print(json.dumps(summary), flush=True)
    lines.append(summary)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")
    if not inside:
        sys.exit("bench_clip_cond_bf16: this tree's fp32 clip lies outside the spread of the parent's two runs")


if __name__ == "__main__":
    main()
