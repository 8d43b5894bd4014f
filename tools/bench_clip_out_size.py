#!/usr/bin/env python3
"""Time images at delivery size (the planar vertical pass of csrc/nca_resize.hip, out_size= of the clip calls) on the GPU and write
profiles/clip_out_size.jsonl.

    python tools/bench_clip_out_size.py [--out profiles/clip_out_size.jsonl] [--other-lib PATH/libncahip.so]

  kernels  32 uint8 images of 256 x 256 -> 1080 x 1080 and -> 1080 x 1920, bicubic and Lanczos, the C calls alone on preallocated buffers,
           device events around one call for all 32 images, median of 10 after 3 warm-ups, per image:
             a  rgb24           ncahip_clip_resize_u8 (two launches)
             b  rgb24+convert   a, then ncahip_clip_rgb_to_yuv420_u8 (three launches; writes 3, reads 3, writes 1.5 bytes per pixel)
             c  i420 / nv12     ncahip_clip_resize_u8_yuv420 (two launches; writes 1.5 bytes per pixel)
           next to the write floor of each arm's final image at the 2.69 TB/s this GPU copies with.  c must not be slower than b (asserted
           before the file is written).
           --other-lib: arm a once more in a child process that loads that library (one built from the parent commit), twice over,
           next to two runs of this tree's: the old path must stay within the spread of the two runs.
  clip     video.stylize_clip over 64 uint8 frames of 256 x 256 on the device, the small single-scale model, step_n = 8, uint8 out; host
           clock between two synchronisations, median of 10 after 3 warm-ups, per frame, twice over: no out_size (also on the other
           library); out_size 1080 x 1080 as rgb24 and as i420 left on the device, delivered to a pinned out= (overlapped), to a pageable
           out=, and by .cpu() after the call.
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
S, N = 256, 32
SIZES = ((1080, 1080), (1080, 1920))
FILTERS = ("bicubic", "lanczos")
F, STEP_N, DELIVERY = 64, 8, (1080, 1080)
COPY_BYTES_PER_US = 2.69e6           # 2.69 TB/s


def timed_events(fn, iters=10, warm=3):
    """median and minimum microseconds of fn between two device events"""
    ts = []
    for i in range(warm + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            ts.append(a.elapsed_time(b) * 1e3)
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


def images():
    return torch.randint(0, 256, (N, S, S, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(DEV)


def resize_call(src, size, filt, rgb):
    """ncahip_clip_resize_u8 alone on preallocated buffers, and what the planar arm shares with it: (call, tables, workspace)"""
    L, st = ops.lib(), ops._stream()
    tx, ty = ops._resize_tables_dev(S, size[1], filt, src.device), ops._resize_tables_dev(S, size[0], filt, src.device)
    need = L.ncahip_clip_resize_workspace(N, S, size[1])
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call():
        return L.ncahip_clip_resize_u8(src.data_ptr(), N, S, S, 0, 0, S, S, tx[0].data_ptr(), tx[1].data_ptr(), tx[0].shape[1], ty[0].data_ptr(),
                                       ty[1].data_ptr(), ty[0].shape[1], rgb.data_ptr(), size[0], size[1], ws.data_ptr(), need, st)

    return call, tx, ty, ws, need


def model():
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    return m


def old_path_rows(emit, label):
    """What --other-lib compares, twice over: arm a of every shape and filter, and stylize_clip without out_size."""
    src = images()
    m = model()
    frames = torch.randint(0, 256, (F, S, S, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    for run in (1, 2):
        for size in SIZES:
            rgb = torch.empty((N,) + size + (3,), dtype=torch.uint8, device=DEV)
            for filt in FILTERS:
                call = resize_call(src, size, filt, rgb)[0]
                assert call() == 0
                med, mn = timed_events(call)
                emit(leg="kernels", arm="a rgb24", library=label, run=run, size=list(size), filter=filt, launches=2, us_per_image=med / N,
                     min_us_per_image=mn / N, write_floor_us=size[0] * size[1] * 3 / COPY_BYTES_PER_US)
            del rgb
        med, mn = timed_sync(lambda: video.stylize_clip(m, frames, step_n=STEP_N, out_dtype=torch.uint8))
        assert video.stylize_clip.last_path == "clip"
        emit(leg="clip", images="grid_rgb24_device", library=label, run=run, frames=F, step_n=STEP_N, us_per_frame=med / F * 1e3,
             min_us_per_frame=mn / F * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_out_size.jsonl"))
    ap.add_argument("--other-lib", default=None, help="a libncahip.so of another commit: its old-path rows are timed in a child process")
    ap.add_argument("--old-path-only", default=None, metavar="LABEL", help="(the child's mode) print the old-path rows under LABEL and stop")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_out_size needs a GPU"
    if args.old_path_only:                                 # an older library lacks the newer exports: bind what it has
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

    if args.old_path_only:
        old_path_rows(emit, args.old_path_only)
        return
    if args.other_lib:
        env = dict(os.environ, NCAHIP_LIB=os.path.abspath(args.other_lib))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--old-path-only", "other"], env=env, check=True, capture_output=True,
                             text=True, timeout=300).stdout
        for line in out.splitlines():
            if line.startswith("{"):
                emit(**json.loads(line))
    old_path_rows(emit, "this")

    # 1. the kernels: b and c
    from ncahip import _capi
    L, st = ops.lib(), ops._stream()
    src = images()
    k = ops.rgb_yuv_coeffs("bt709", "limited")
    slower = []
    for size in SIZES:
        rgb = torch.empty((N,) + size + (3,), dtype=torch.uint8, device=DEV)
        two_img, fused_img = (torch.empty(N, 3 * size[0] // 2, size[1], dtype=torch.uint8, device=DEV) for _ in range(2))
        floor = size[0] * size[1] * 1.5 / COPY_BYTES_PER_US
        for filt in FILTERS:
            to_rgb, tx, ty, ws, need = resize_call(src, size, filt, rgb)
            for fmt in ("i420", "nv12"):
                layout = _capi.YUV_LAYOUTS[fmt]

                def two(layout=layout):
                    to_rgb()
                    return L.ncahip_clip_rgb_to_yuv420_u8(rgb.data_ptr(), layout, N, size[0], size[1], k.ctypes.data, two_img.data_ptr(), st)

                def fused(layout=layout):
                    return L.ncahip_clip_resize_u8_yuv420(src.data_ptr(), N, S, S, 0, 0, S, S, tx[0].data_ptr(), tx[1].data_ptr(), tx[0].shape[1],
                                                          ty[0].data_ptr(), ty[1].data_ptr(), ty[0].shape[1], layout, k.ctypes.data,
                                                          fused_img.data_ptr(), size[0], size[1], ws.data_ptr(), need, st)

                assert two() == 0 and fused() == 0
                assert torch.equal(fused_img, two_img), (size, filt, fmt)                # what is timed is right
                res = {}
                for run in (1, 2):
                    res.setdefault("b", []).append(timed_events(two))
                    res.setdefault("c", []).append(timed_events(fused))
                for arm, name, launches in (("b", f"b rgb24+convert {fmt}", 3), ("c", f"c {fmt}", 2)):
                    emit(leg="kernels", arm=name, size=list(size), filter=filt, launches=launches, us_per_image=[t[0] / N for t in res[arm]],
                         min_us_per_image=[t[1] / N for t in res[arm]], write_floor_us=floor)
                if max(t[0] for t in res["c"]) > min(t[0] for t in res["b"]):
                    slower.append((size, filt, fmt, res))
        del rgb, two_img, fused_img
    ops.check_errors()

    # 2. stylize_clip end to end at delivery size
    m = model()
    frames = torch.randint(0, 256, (F, S, S, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).to(DEV)
    h, w = DELIVERY
    legs = []
    for name, kw, shape in (("rgb24", {}, (F, h, w, 3)), ("i420", {"out_format": "i420"}, (F, 3 * h // 2, w))):
        def call(kw=kw, **more):                     # every call from the same fire-mask position: the same images
            m._mask_step = 0
            return video.stylize_clip(m, frames, step_n=STEP_N, out_dtype=torch.uint8, out_size=DELIVERY, **kw, **more)

        pageable, pinned = torch.empty(shape, dtype=torch.uint8), torch.empty(shape, dtype=torch.uint8).pin_memory()
        want = call()[0].cpu()
        for out in (pageable, pinned):
            assert torch.equal(call(out=out)[0], want), name                       # what is timed is right
        del want
        legs += [(f"{name}_device", lambda call=call: call(), None),
                 (f"{name}_pinned_out", lambda call=call, o=pinned: call(out=o), "overlapped"),
                 (f"{name}_pinned_out_per_call_8", lambda call=call, o=pinned: call(out=o, frames_per_call=8), "overlapped"),
                 (f"{name}_pageable_out", lambda call=call, o=pageable: call(out=o), "sync"),
                 (f"{name}_cpu_after", lambda call=call: call()[0].cpu(), None)]
    res = {}
    for run in (1, 2):                                   # twice over: the two figures of a leg give the session's spread
        for name, fn, download in legs:
            med, mn = timed_sync(fn)
            assert video.stylize_clip.last_download == download and video.stylize_clip.last_path == "clip", name
            res.setdefault(name, []).append(med / F * 1e3)
    ops.check_errors()
    emit(leg="clip", model="DyNCA C=12 fc=96 edges [0]", frames=F, frames_per_call=32, step_n=STEP_N, size=[S, S], out_size=list(DELIVERY),
         bytes_per_image={"rgb24": h * w * 3, "i420": h * w * 3 // 2}, us_per_frame=res)

    assert not slower, f"the planar pass is slower than resize + convert: {slower}"      # a failing run leaves no profile behind
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
