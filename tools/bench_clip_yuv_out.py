#!/usr/bin/env python3
"""Time planar YUV 4:2:0 images out of the clip calls (csrc/nca_yuv_out.hip, the planar emit of csrc/nca_clip.hip) and the overlapped
download into a pinned buffer on the GPU, and write profiles/clip_yuv_out.jsonl.

    python tools/bench_clip_yuv_out.py [--out profiles/clip_yuv_out.jsonl] [--other-lib PATH/libncahip.so]

  emit     one image out of a state of 1 x 12 x 256^2 (ncahip_clip_emit) and of 1 x 20 x 256^2 (ncahip_clip_emit_unit), per launch:
             rgb24          the uint8 RGB emit
             i420 / nv12    the fused planar emit (one launch, no RGB image)
             rgb24+convert  the uint8 RGB emit followed by ncahip_clip_rgb_to_yuv420_u8 (two launches)
           A launch takes a few microseconds, less than the host needs to enqueue it, so the launches are timed back to back: the stream
           is first kept busy with matrix products, 50 launches queue up behind them, and device events around the 50 give the time per
           queued launch (the gaps between consecutive kernels included: not one kernel's duration alone).  Median of 10 such samples.
           --other-lib: the rgb24 rows once more in a child process that loads that library (one built from the parent commit), twice
           over, next to two runs of this tree's -- the RGB24 emit must stay within the spread of the other's two runs.
  stylize  video.stylize_clip over 64 uint8 frames of 256 x 256 on the device, the small single-scale model, step_n = 8, uint8 out; host
           clock between two synchronisations, median of 10, per frame, twice over: RGB24 and I420 images left on the device (RGB24 also on
           the other library), then brought to the host by .cpu() after the call, by out=<pageable tensor>, by out=<pinned tensor>
           (downloads on the side stream, chunk k while chunk k + 1 computes) and by the pinned tensor at frames_per_call = 8.
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
S, BATCH = 256, 50
F, STEP_N = 64, 8


def timed_queued(fn, busy, iters=10, warm=2):
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


def timed_sync(fn, iters=10, warm=3):
    """median and minimum ms of fn on the host clock between two device synchronisations (for callables with a host part: downloads)"""
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


def states():
    gen = torch.Generator().manual_seed(0)
    return {12: (torch.rand(1, 12, S, S, generator=gen) * 1.5 - 0.75).to(DEV), 20: (torch.rand(1, 20, S, S, generator=gen) * 1.4 - 0.2).to(DEV)}


def emitter(x, fmt_word, img):
    """The C call alone on preallocated buffers: ncahip_clip_emit for C = 12, ncahip_clip_emit_unit for C = 20."""
    L, st = ops.lib(), ops._stream()
    C = x.shape[1]
    if C == 12:
        return lambda: L.ncahip_clip_emit(x.data_ptr(), img.data_ptr(), fmt_word, 1, C, 3, S, S, st)
    return lambda: L.ncahip_clip_emit_unit(x.data_ptr(), img.data_ptr(), fmt_word, 1, C, S, S, st)


def model():
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    return m


def rgb24_rows(emit, label, busy):
    """What --other-lib compares, twice over: the uint8 RGB emit of both shapes and stylize_clip with RGB24 images left on the device."""
    xs = states()
    m = model()
    frames = torch.randint(0, 256, (F, S, S, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    for run in (1, 2):
        for C, x in xs.items():
            img = torch.empty(1, S, S, 3, dtype=torch.uint8, device=DEV)
            fn = emitter(x, 1, img)
            assert fn() == 0
            med, mn = timed_queued(fn, busy)
            emit(leg="emit", image="rgb24", library=label, run=run, shape=[1, C, S, S], launches=1, us_per_image=med, min_us_per_image=mn)
        med, mn = timed_sync(lambda: video.stylize_clip(m, frames, step_n=STEP_N, out_dtype=torch.uint8))
        assert video.stylize_clip.last_path == "clip"
        emit(leg="stylize", images="rgb24_device", library=label, run=run, frames=F, step_n=STEP_N, us_per_frame=med / F * 1e3,
             min_us_per_frame=mn / F * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_yuv_out.jsonl"))
    ap.add_argument("--other-lib", default=None, help="a libncahip.so of another commit: its RGB24 rows are timed in a child process")
    ap.add_argument("--rgb24-only", default=None, metavar="LABEL", help="(the child's mode) print the rgb24 rows under LABEL and stop")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_yuv_out needs a GPU"
    if args.rgb24_only:                                    # an older library lacks the newer exports: bind what it has
        import ctypes
        from ncahip import _capi
        probe = ctypes.CDLL(_capi.LIB_PATH)
        for name in [n for n in _capi.SIGNATURES if not hasattr(probe, n)]:
            del _capi.SIGNATURES[name]
    ops.selftest()
    busy = torch.randn(4096, 4096, device=DEV)
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    if args.rgb24_only:
        rgb24_rows(emit, args.rgb24_only, busy)
        return

    if args.other_lib:
        env = dict(os.environ, NCAHIP_LIB=os.path.abspath(args.other_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--rgb24-only", "other"], env=env, check=True, capture_output=True,
                             text=True, timeout=300).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    rgb24_rows(emit, "this", busy)

    # 1. the image output alone
    from ncahip import _capi
    L, st = ops.lib(), ops._stream()
    for C, x in states().items():
        rgb = torch.empty(1, S, S, 3, dtype=torch.uint8, device=DEV)
        to_rgb = emitter(x, 1, rgb)
        for fmt in ("i420", "nv12"):
            k = ops.rgb_yuv_coeffs("bt709", "limited")
            word = _capi.clip_yuv420(_capi.YUV_LAYOUTS[fmt], 1, 0)
            fused_img, two_img = (torch.empty(1, 3 * S // 2, S, dtype=torch.uint8, device=DEV) for _ in range(2))
            fused = emitter(x, word, fused_img)

            def two(k=k, fmt=fmt, two_img=two_img):
                to_rgb()
                return L.ncahip_clip_rgb_to_yuv420_u8(rgb.data_ptr(), _capi.YUV_LAYOUTS[fmt], 1, S, S, k.ctypes.data, two_img.data_ptr(), st)

            assert fused() == 0 and two() == 0
            assert torch.equal(fused_img, two_img) and torch.equal(fused_img.cpu(), ops.rgb_to_yuv420_host(rgb.cpu(), fmt)), (C, fmt)   # what is timed is right
            med, mn = timed_queued(fused, busy)
            emit(leg="emit", image=fmt, shape=[1, C, S, S], launches=1, us_per_image=med, min_us_per_image=mn)
            med, mn = timed_queued(two, busy)
            emit(leg="emit", image=f"rgb24+convert {fmt}", shape=[1, C, S, S], launches=2, us_per_image=med, min_us_per_image=mn)
    ops.check_errors()

    # 2. stylize_clip end to end, the images left on the device or brought to the host
    m = model()
    frames = torch.randint(0, 256, (F, S, S, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    legs = []
    for name, kw, shape in (("rgb24", {}, (F, S, S, 3)), ("i420", {"out_format": "i420"}, (F, 3 * S // 2, S))):
        def call(kw=kw, **more):                     # every call from the same fire-mask position: the same images
            m._mask_step = 0
            return video.stylize_clip(m, frames, step_n=STEP_N, out_dtype=torch.uint8, **kw, **more)

        pageable, pinned = torch.empty(shape, dtype=torch.uint8), torch.empty(shape, dtype=torch.uint8).pin_memory()
        want = call()[0].cpu()
        for out in (pageable, pinned):
            assert torch.equal(call(out=out)[0], want), name                       # what is timed is right
        if name == "i420":
            legs.append((f"{name}_device", lambda call=call: call(), None))
        legs += [(f"{name}_cpu_after", lambda call=call: call()[0].cpu(), None),
                 (f"{name}_pageable_out", lambda call=call, o=pageable: call(out=o), "sync"),
                 (f"{name}_pinned_out", lambda call=call, o=pinned: call(out=o), "overlapped"),
                 (f"{name}_pinned_out_per_call_8", lambda call=call, o=pinned: call(out=o, frames_per_call=8), "overlapped"),
                 (f"{name}_device_per_call_8", lambda call=call: call(frames_per_call=8), None)]
    res = {}
    for run in (1, 2):                                   # twice over: the two figures of a leg give the session's spread
        for name, fn, download in legs:
            med, mn = timed_sync(fn)
            assert video.stylize_clip.last_download == download and video.stylize_clip.last_path == "clip", name
            res.setdefault(name, []).append(med / F * 1e3)
    ops.check_errors()
    emit(leg="stylize", model="DyNCA C=12 fc=96 edges [0]", frames=F, frames_per_call=32, step_n=STEP_N, size=[S, S],
         bytes_per_image={"rgb24": S * S * 3, "i420": S * S * 3 // 2}, us_per_frame=res)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
