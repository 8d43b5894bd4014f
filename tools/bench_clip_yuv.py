#!/usr/bin/env python3
"""Time planar YUV 4:2:0 clip frames (csrc/nca_yuv.hip, the planar loader of csrc/nca_resize.hip) and the overlapped upload of pinned
frames on the GPU, and write profiles/clip_yuv.jsonl.

    python tools/bench_clip_yuv.py [--out profiles/clip_yuv.jsonl] [--other-lib PATH/libncahip.so]

  preprocess  32 frames of 1080 x 1920 -> 256 x 256, both reference crops, both filters, device events around the launches alone, median
              of 10 after 3 warm-ups, per frame:
                rgb24            ops.clip_resize on RGB24 frames (two launches; 6.2 MB per frame in)
                i420 / nv12      ops.clip_resize_yuv420 (the same two launches, the conversion in the horizontal pass's loader; 3.1 MB in)
                convert_resize   ops.yuv420_to_rgb (I420) followed by ops.clip_resize: three launches and a full-size RGB image between
              --other-lib: the rgb24 rows once more in a child process that loads that library (one built from the parent commit),
              twice over, next to two runs of this tree's -- the RGB24 instantiation must stay within the spread of the other's two runs.
  stylize     video.stylize_clip(size=(256, 256)) over 64 frames of 1080p, the small single-scale model, step_n = 8, uint8 out; host
              clock between two synchronisations, median of 10, per frame: RGB24 and I420 frames on the device, in pageable and in pinned
              host memory (pinned: uploads on the side stream, chunk k + 1 while chunk k computes), the pinned legs also at
              frames_per_call = 8 (eight chunks instead of two: more of the upload has a computing chunk to hide behind).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]
import torch

from ncahip import ops, video

DEV = "cuda"
N, H, W, S = 32, 1080, 1920, 256
CASES = (("dynca", "bicubic"), ("dynca", "lanczos"), ("conditioned", "bicubic"), ("conditioned", "lanczos"))


def timed(fn, iters=10, warm=3):
    """median and minimum ms of fn, device events around each call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def timed_sync(fn, iters=10, warm=3):
    """as timed, on the host clock between two device synchronisations (for callables with a host part: uploads)"""
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


def planar(n, seed):
    """n random planar frames [n, 3H/2, W] on the host: random planes, so the two layouts have the same size and statistics"""
    return torch.randint(0, 256, (n, 3 * H // 2, W), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def rgb24_rows(emit, label):
    """The RGB24 resize alone, twice over: what --other-lib compares."""
    frames = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8).to(DEV)
    for run in (1, 2):
        for kind, filt in CASES:
            box = video.reference_crop(kind, H, W)
            med, mn = timed(lambda: ops.clip_resize(frames, (S, S), box, filt))
            emit(leg="preprocess", source="rgb24", library=label, run=run, crop=kind, resample=filt, frames=N, us_per_frame=med / N * 1e3,
                 min_us_per_frame=mn / N * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_yuv.jsonl"))
    ap.add_argument("--other-lib", default=None, help="a libncahip.so of another commit: its RGB24 resize is timed in a child process")
    ap.add_argument("--rgb24-only", default=None, metavar="LABEL", help="(the child's mode) print the rgb24 rows under LABEL and stop")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_yuv needs a GPU"
    if args.rgb24_only:                                    # an older library lacks the newer exports: bind what it has
        import ctypes
        from ncahip import _capi
        probe = ctypes.CDLL(_capi.LIB_PATH)
        for name in [n for n in _capi.SIGNATURES if not hasattr(probe, n)]:
            del _capi.SIGNATURES[name]
    ops.selftest()
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    if args.rgb24_only:
        rgb24_rows(emit, args.rgb24_only)
        return

    # 1. the preprocessing launches alone
    if args.other_lib:
        env = dict(os.environ, NCAHIP_LIB=os.path.abspath(args.other_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rgb24-only", "other"], env=env, check=True, capture_output=True,
                             text=True, timeout=300).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    rgb24_rows(emit, "this")
    for fmt in ("i420", "nv12"):
        frames = planar(N, 1).to(DEV)
        for kind, filt in CASES:
            box = video.reference_crop(kind, H, W)
            med, mn = timed(lambda: ops.clip_resize_yuv420(frames, (S, S), box, filt, fmt))
            two = lambda: ops.clip_resize(ops.yuv420_to_rgb(frames, fmt, crop=box), (S, S), None, filt)      # noqa: E731
            assert torch.equal(ops.clip_resize_yuv420(frames[:2], (S, S), box, filt, fmt), two()[:2]), (fmt, kind, filt)   # what is timed is right
            emit(leg="preprocess", source=fmt, crop=kind, resample=filt, frames=N, us_per_frame=med / N * 1e3, min_us_per_frame=mn / N * 1e3)
            if fmt == "i420":
                med, mn = timed(two)
                cmed, _ = timed(lambda: ops.yuv420_to_rgb(frames, fmt, crop=box))
                emit(leg="preprocess", source="i420 convert_resize", crop=kind, resample=filt, frames=N, us_per_frame=med / N * 1e3,
                     min_us_per_frame=mn / N * 1e3, conversion_alone_us_per_frame=cmed / N * 1e3)
        del frames
    ops.check_errors()

    # 2. stylize_clip(size=...) end to end
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    F, step_n = 64, 8
    rgb = torch.randint(0, 256, (F, H, W, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    yuv = planar(F, 3)
    sources = {"rgb24": (rgb, {}), "i420": (yuv, {"pixel_format": "i420"})}
    legs = []
    for name, (host, kw) in sources.items():
        call = lambda fr, kw=kw, **more: video.stylize_clip(m, fr, step_n=step_n, out_dtype=torch.uint8, size=(S, S), **kw, **more)      # noqa: E731
        dev, pinned = host.to(DEV), host.pin_memory()
        legs += [(f"{name}_device", lambda call=call, dev=dev: call(dev), "sync"),
                 (f"{name}_pageable", lambda call=call, host=host: call(host), "sync"),
                 (f"{name}_pinned", lambda call=call, pinned=pinned: call(pinned), "overlapped"),
                 (f"{name}_pinned_per_call_8", lambda call=call, pinned=pinned: call(pinned, frames_per_call=8), "overlapped"),
                 (f"{name}_device_per_call_8", lambda call=call, dev=dev: call(dev, frames_per_call=8), "sync")]
    res = {}
    for run in (1, 2):                                   # twice over: the two figures of a leg give the session's spread
        for name, fn, upload in legs:
            med, mn = timed_sync(fn)
            assert video.stylize_clip.last_upload == upload and video.stylize_clip.last_path == "clip", name
            res.setdefault(name, []).append(med / F * 1e3)
    ops.check_errors()
    emit(leg="stylize", model="DyNCA C=12 fc=96 edges [0]", frames=F, frames_per_call=32, step_n=step_n, src=[H, W], size=[S, S], crop="dynca",
         resample="bicubic", bytes_per_frame={"rgb24": H * W * 3, "i420": H * W * 3 // 2}, us_per_frame=res)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
