#!/usr/bin/env python3
"""Time the crop + resize of decoder-sized uint8 frames (csrc/nca_resize.hip) on the GPU and write profiles/clip_resize.jsonl.

    python tools/bench_clip_resize.py [--out profiles/clip_resize.jsonl]

32 frames of 1080 x 1920 -> 256 x 256, both filters, both reference crops.  Device events around each callable, median of 10 after 3
warm-ups, reported per frame.

  resize     ops.clip_resize alone (its two launches), next to
               floor_us       the bytes the horizontal pass must read (the crop) over this device's measured copy rate (a 256 MiB
                              device-to-device copy_: bytes copied per second),
               interpolate_us torch's F.interpolate(mode='bicubic', antialias=True) on the same crop as float32 [N,3,h,w] -- a yardstick
                              only: its arithmetic differs (float, no uint8 between the passes) and the conversion to float is not in it.
  stylize    video.stylize_clip(size=(256, 256)) on the 1080p frames against video.stylize_clip on frames resized beforehand (what the
             library could do before), frames on the device, uint8 out; the difference is what the feature costs per frame.  The same with
             the frames on the host (pageable memory), where the upload of the native-size frames is part of the call.
  pillow     if Pillow is installed: its own per-frame host resize of the same crop, for context.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-stylization-with-nca_amd")]
import torch
import torch.nn.functional as F

from ncahip import ops, video

DEV = "cuda"
N, H, W, S = 32, 1080, 1920, 256


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_resize.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip_resize needs a GPU"
    ops.selftest()
    lines = []

    def emit(**kw):
        print(json.dumps(kw), flush=True)
        lines.append(kw)

    gen = torch.Generator().manual_seed(0)
    host = torch.randint(0, 256, (N, H, W, 3), generator=gen, dtype=torch.uint8)
    frames = host.to(DEV)

    # this device's copy rate
    big = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(big)
    med, _ = timed(lambda: dst.copy_(big))
    copy_rate = big.numel() / (med * 1e-3)            # bytes copied per second
    emit(leg="copy_rate", bytes=big.numel(), ms=med, GB_per_s=copy_rate / 1e9)
    del big, dst

    # 1. the resize launches alone
    for kind, filt in (("dynca", "bicubic"), ("dynca", "lanczos"), ("conditioned", "bicubic"), ("conditioned", "lanczos")):
        box = video.reference_crop(kind, H, W)
        x0, y0, cw, ch = box
        med, mn = timed(lambda: ops.clip_resize(frames, (S, S), box, filt))
        got = ops.clip_resize(frames[:2], (S, S), box, filt).cpu()
        assert torch.equal(got, ops.clip_resize_host(host[:2], (S, S), box, filt)), (kind, filt)       # what is timed is right
        crop_f32 = frames[:, y0:y0 + ch, x0:x0 + cw].permute(0, 3, 1, 2).float().contiguous()
        imed, _ = timed(lambda: F.interpolate(crop_f32, size=(S, S), mode="bicubic", antialias=True))
        del crop_f32
        read = N * ch * cw * 3
        kx, _ = ops.resize_tables(cw, S, filt)
        emit(leg="resize", crop=kind, box=list(box), resample=filt, frames=N, src=[H, W], size=[S, S], taps=int(kx.shape[1]),
             us_per_frame=med / N * 1e3, min_us_per_frame=mn / N * 1e3, bytes_read_per_frame=read // N,
             floor_us_per_frame=read / copy_rate / N * 1e6, interpolate_bicubic_antialias_us_per_frame=imed / N * 1e3)
    ops.check_errors()

    # 2. stylize_clip(size=...) against stylize_clip on frames resized beforehand
    from ncahip.models.dynca import DyNCA
    torch.manual_seed(0)
    m = DyNCA(12, 3, fc_dim=96, padding_mode="circular", conditioning="edges", edge_transform="tanh", perception_scales=[0],
              device=torch.device(DEV))
    m.mask_rng, m.mask_seed = "philox", 1
    small = video.resize_frames(frames, (S, S), "dynca", "bicubic")
    small_host = small.cpu()
    step_n = 8
    legs = [("resized_beforehand_device", lambda: video.stylize_clip(m, small, step_n=step_n, out_dtype=torch.uint8)),
            ("size_device", lambda: video.stylize_clip(m, frames, step_n=step_n, out_dtype=torch.uint8, size=(S, S))),
            ("resized_beforehand_host", lambda: video.stylize_clip(m, small_host, step_n=step_n, out_dtype=torch.uint8)),
            ("size_host", lambda: video.stylize_clip(m, host, step_n=step_n, out_dtype=torch.uint8, size=(S, S)))]
    res = {}
    for run in (1, 2):                                   # twice over: the two figures of a leg give the session's spread
        for name, fn in legs:
            med, mn = timed_sync(fn)
            res.setdefault(name, []).append(med / N * 1e3)
    ops.check_errors()
    emit(leg="stylize", model="DyNCA C=12 fc=96 edges [0]", frames=N, step_n=step_n, src=[H, W], size=[S, S], crop="dynca", resample="bicubic",
         us_per_frame={k: v for k, v in res.items()},
         feature_cost_us_per_frame_device=min(res["size_device"]) - min(res["resized_beforehand_device"]),
         feature_cost_us_per_frame_host=min(res["size_host"]) - min(res["resized_beforehand_host"]))

    # 3. Pillow on the host, for context
    try:
        from PIL import Image
    except ImportError:
        emit(leg="pillow", error="Pillow is not installed here")
    else:
        import PIL
        for kind, filt, pf in (("dynca", "bicubic", Image.BICUBIC), ("conditioned", "lanczos", Image.LANCZOS)):
            x0, y0, cw, ch = video.reference_crop(kind, H, W)
            arr = host[0].numpy()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                out = Image.fromarray(arr[y0:y0 + ch, x0:x0 + cw]).resize((S, S), pf)
                ts.append((time.perf_counter() - t0) * 1e6)
            assert out.size == (S, S)
            emit(leg="pillow", version=PIL.__version__, crop=kind, resample=filt, us_per_frame=statistics.median(ts))

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
