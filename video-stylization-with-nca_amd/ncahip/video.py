"""Frame-conditioned video synthesis loop.

Reference: ConditioneDyNCA/utils/misc/video_utils.py:50-83 (`save_video`): seed once, then for every target frame run
`steps_per_frame` x `forward_nsteps(h, step_n, cond_img=gray(frame))` and emit `clip(rgb, -1, 1) * 0.5 + 0.5`.  Video
decoding / encoding (moviepy, cv2) is outside the hot path: frames come in and go out as tensors.

stylize_clip also serves the ExtraChannels family (ncahip.models.dynca_extra.DyNCA), whose loop
(ExtraChannels/utils/misc/video_utils.py:66-82) appends the grey frame to the state as its last channel before every call and
drops it again after.

Decoder-sized frames: reference_crop / resize_frames are the reference's host-side shrink (Pillow: centre crop, then an 8-bit
Image.resize) on the device, bit for bit; stylize_clip(size=...) and stylize_clip_conditioned(size=...) apply it per chunk.

Planar frames: a decoder writes YUV 4:2:0 (I420 or NV12), not RGB24.  pixel_format='i420' / 'nv12' hands such frames to the same entry
points; the conversion (include/ncahip.h, "planar YUV frames") runs on the device, inside the resize's loader when size is set.  Pinned
host frames are uploaded on a side stream, chunk k + 1 while chunk k computes (_chunks).

Planar images: a video encoder takes YUV 4:2:0 as well.  out_format='i420' / 'nv12' makes the clip entry points write it straight from
the state (include/ncahip.h, "planar YUV images"), and out=<pinned host tensor> delivers the images into the caller's buffer on a second
side stream, chunk k while chunk k + 1 computes (_Downloads).
"""
import contextlib
import operator
from typing import Iterable, Iterator, Optional

import torch


def rgb_to_grayscale(x: torch.Tensor) -> torch.Tensor:
    """ITU-R 601 luma as torchvision's rgb_to_grayscale (the reference's RGBToGrayscale): [B,3,H,W] -> [B,1,H,W].
    (preprocess_texture.py:178-179 takes the channel mean instead: stylize_clip offers both and defaults to the mean.)"""
    r, g, b = x.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(-3)


@torch.no_grad()
def synthesize_video(nca_model, frames: Iterable[torch.Tensor], step_n: int = 8, steps_per_frame: int = 1,
                     size=None, state: Optional[torch.Tensor] = None) -> Iterator[torch.Tensor]:
    """Yields one [3,H,W] image in [0,1] per (frame, k): video_utils.py:66-83.  `frames`: tensors [3,H,W] in [-1,1] on
    the model's device (the reference's preprocess_video output, one time slice each).  The NCA state persists across
    frames; pass `state` to continue a previous call.
    (stylize_clip runs a whole clip per call; it conditions on the channel-mean grey by default, this loop on the luma.)"""
    h = state
    for frame in frames:
        frame = frame.to(nca_model.device)
        if h is None:
            hh, ww = frame.shape[-2:]
            h = nca_model.seed(1, size=size if size is not None else (ww, hh))
        cond = rgb_to_grayscale(frame.unsqueeze(0))
        for _ in range(int(steps_per_frame)):
            h, rgb = nca_model.forward_nsteps(h, step_n, cond_img=cond)
            yield (rgb[0].clamp(-1.0, 1.0) + 1.0) / 2.0
    synthesize_video.last_state = h


def _gray(x: torch.Tensor, gray: str) -> torch.Tensor:
    """[B,3,H,W] -> [B,1,H,W]: 'mean' = the reference's RGBToGrayscale (preprocess_texture.py:178-179), 'luma' = rgb_to_grayscale."""
    if gray == "mean":
        return x.mean(dim=-3, keepdim=True)
    if gray == "luma":
        return rgb_to_grayscale(x)
    raise ValueError(f"gray must be 'mean' or 'luma', got {gray!r}")


def _widen(frames: torch.Tensor) -> torch.Tensor:
    """[n,H,W,3] uint8 -> [n,3,H,W] float32 in [-1, 1], as the reference's preprocessing (preprocess_texture.py:28, :54)."""
    return (frames.float() / 255.0 * 2.0 - 1.0).permute(0, 3, 1, 2).contiguous()


def _extra_channels(nca_model) -> bool:
    """True for the ExtraChannels family: the grey frame is the model's last state channel, not a cond_img."""
    from .models import dynca_extra
    return isinstance(nca_model, dynca_extra.DyNCA)


def _clip_route(nca_model, h: torch.Tensor) -> bool:
    """True when ncahip_dynca_clip_f32 (edge conditioning) or ncahip_dynca_clip_xc_f32 (an extra-channel model) covers the model:
    perception_scales [0] or the fused [0, 1], an fp32 state on the GPU, one sample."""
    if not (_extra_channels(nca_model) or getattr(nca_model, "conditioning", None) == "edges"):
        return False
    if not h.is_cuda or h.dtype != torch.float32 or h.shape[0] != 1:
        return False
    scales = list(getattr(nca_model, "perception_scales", [0]))
    return scales == [0] or (scales == [0, 1] and nca_model._two_scale_fused(h))


def reference_crop(kind: str, H: int, W: int):
    """The crop box (x0, y0, w, h) the reference takes out of an H x W frame before it resizes.
    'dynca' (preprocess_texture.py:17-25): a square frame is kept whole; otherwise cut = |W - H| // 2 comes off both ends of the
    longer side -- an odd difference leaves that side one pixel longer than the other, as the reference does.
    'conditioned' (EncoderConditioning/utils/utils.py:10-16): n = min(W, H), columns (W - n) // 2 .. (W + n) // 2, rows likewise."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"reference_crop: the frame must be at least 1 x 1, got {H} x {W}")
    if kind == "dynca":
        cut = abs(W - H) // 2
        return (cut, 0, W - 2 * cut, H) if W > H else (0, cut, W, H - 2 * cut)
    if kind == "conditioned":
        n = min(W, H)
        left, top = (W - n) // 2, (H - n) // 2
        return (left, top, (W + n) // 2 - left, (H + n) // 2 - top)
    raise ValueError(f"crop kind must be 'dynca' or 'conditioned', got {kind!r}")


PIXEL_FORMATS = ("rgb24", "i420", "nv12")


def _planar(frames: torch.Tensor, pixel_format, yuv_matrix, yuv_range):
    """None for pixel_format 'rgb24'; for 'i420' / 'nv12' the frames' (h, w), after validating the frames ([F, 3h/2, w] uint8, even h and w),
    the matrix and the range.  ValueError for anything else, before anything runs."""
    from . import ops
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format must be one of {PIXEL_FORMATS}, got {pixel_format!r}")
    if pixel_format == "rgb24":
        return None
    ops.yuv_coeffs(yuv_matrix, yuv_range)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"pixel_format={pixel_format!r} takes uint8 frames [F, 3h/2, w] (what the decoder wrote), got {getattr(frames, 'dtype', type(frames))}")
    return ops.yuv420_frame_size(tuple(frames.shape))


def yuv420_to_rgb(frames: torch.Tensor, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited") -> torch.Tensor:
    """Planar YUV 4:2:0 frames [N, 3h/2, w] uint8 ('i420': Y, U, V planes; 'nv12': Y plane, interleaved UV rows) -> RGB [N,h,w,3] uint8 on
    the frames' device, by include/ncahip.h's integer arithmetic with nearest chroma.  yuv_matrix 'bt601' or 'bt709', yuv_range 'limited'
    or 'full'.  CUDA frames run ncahip_clip_yuv420_to_rgb_u8 (one launch), CPU frames its numpy mirror ops.yuv420_to_rgb_host."""
    from . import ops
    if _planar(frames, pixel_format, yuv_matrix, yuv_range) is None:
        raise ValueError(f"pixel_format must be 'i420' or 'nv12', got {pixel_format!r}")
    return (ops.yuv420_to_rgb if frames.is_cuda else ops.yuv420_to_rgb_host)(frames, pixel_format, yuv_matrix, yuv_range)


def rgb_to_yuv420(frames: torch.Tensor, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited") -> torch.Tensor:
    """RGB24 images [N,h,w,3] uint8 (even h and w) -> planar YUV 4:2:0 [N, 3h/2, w] uint8 ('i420' or 'nv12') on the images' device, by
    include/ncahip.h's integer arithmetic; the chroma sample of a 2 x 2 block is its mean.  CUDA images run ncahip_clip_rgb_to_yuv420_u8
    (one launch), CPU images its numpy mirror ops.rgb_to_yuv420_host.  What out_format= of the clip calls writes without the RGB image."""
    from . import ops
    if pixel_format not in ("i420", "nv12"):
        raise ValueError(f"pixel_format must be 'i420' or 'nv12', got {pixel_format!r}")
    ops.rgb_yuv_coeffs(yuv_matrix, yuv_range)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError(f"rgb_to_yuv420 takes uint8 images [N,h,w,3], got {getattr(frames, 'dtype', type(frames))}")
    ops._rgb_images_shape(tuple(frames.shape))
    return (ops.rgb_to_yuv420 if frames.is_cuda else ops.rgb_to_yuv420_host)(frames, pixel_format, yuv_matrix, yuv_range)


def resize_frames(frames: torch.Tensor, size, crop=None, resample: str = "bicubic", pixel_format: str = "rgb24", yuv_matrix: str = "bt709",
                  yuv_range: str = "limited", out_format: str = "rgb24", out_yuv_matrix: str = "bt709",
                  out_yuv_range: str = "limited") -> torch.Tensor:
    """frames [N,H,W,3] uint8 -> [N,out_h,out_w,3] uint8 on the frames' device: the reference's crop, then Pillow's 8-bit Image.resize,
    bit for bit.  size = (out_h, out_w) -- rows first; the reference hands Pillow (x, y).  crop: 'dynca' or 'conditioned'
    (reference_crop), None (the whole frame) or a box (x0, y0, w, h).  resample: 'bicubic' (Image.resize's default, what
    preprocess_style_image gets) or 'lanczos' (load_image).  CUDA frames run ncahip_clip_resize_u8 (two launches for all N frames), CPU
    frames its numpy mirror ops.clip_resize_host on the same tables.
    pixel_format 'i420' / 'nv12': frames are planar YUV 4:2:0 [N, 3h/2, w] uint8 (yuv420_to_rgb); the result is resize_frames of their
    RGB, bit for bit.  CUDA frames run ncahip_clip_resize_yuv420_u8 (the conversion inside the horizontal pass's loader, no full-size
    RGB image), CPU frames the two mirrors.
    out_format 'i420' / 'nv12' (even out_h and out_w): the result as planar YUV 4:2:0 [N, 3 out_h / 2, out_w] uint8 -- rgb_to_yuv420(the
    'rgb24' result, out_format, out_yuv_matrix, out_yuv_range), bit for bit.  CUDA RGB24 frames run ncahip_clip_resize_u8_yuv420 (the
    vertical pass writes the planes, no full-size RGB image), CPU frames ops.clip_resize_to_yuv420_host; planar frames convert the
    resized image."""
    from . import ops
    if out_format not in ops.OUT_FORMATS:
        raise ValueError(f"out_format must be one of {ops.OUT_FORMATS}, got {out_format!r}")
    if out_format != "rgb24":
        ops.rgb_yuv_coeffs(out_yuv_matrix, out_yuv_range)
        ops._even_size(size, "resize_frames")
        if pixel_format != "rgb24":
            return rgb_to_yuv420(resize_frames(frames, size, crop, resample, pixel_format, yuv_matrix, yuv_range), out_format, out_yuv_matrix,
                                 out_yuv_range)
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"frames must be a uint8 tensor [N,H,W,3] (the reference resizes 8-bit images), got "
                             f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)} {getattr(frames, 'dtype', '')}")
        if isinstance(crop, str):
            crop = reference_crop(crop, frames.shape[1], frames.shape[2])
        return (ops.clip_resize_to_yuv420 if frames.is_cuda else ops.clip_resize_to_yuv420_host)(frames, size, crop, resample, out_format,
                                                                                                out_yuv_matrix, out_yuv_range)
    planar = _planar(frames, pixel_format, yuv_matrix, yuv_range)
    if planar is not None:
        if isinstance(crop, str):
            crop = reference_crop(crop, *planar)
        if frames.is_cuda:
            return ops.clip_resize_yuv420(frames, size, crop, resample, pixel_format, yuv_matrix, yuv_range)
        ops._resize_filter(resample)
        ops._resize_args((frames.shape[0],) + planar + (3,), size, crop)           # bad size / crop: before the conversion
        return ops.clip_resize_host(ops.yuv420_to_rgb_host(frames, pixel_format, yuv_matrix, yuv_range, crop), size, None, resample)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
        raise ValueError(f"frames must be a uint8 tensor [N,H,W,3] (the reference resizes 8-bit images), got "
                         f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)} {getattr(frames, 'dtype', '')}")
    if isinstance(crop, str):
        crop = reference_crop(crop, frames.shape[1], frames.shape[2])
    return (ops.clip_resize if frames.is_cuda else ops.clip_resize_host)(frames, size, crop, resample)


def _sized(frames: torch.Tensor, size, planar=None):
    """stylize_clip*(size=...): the model grid (H, W) after validating the frames the resize takes (planar frames: _planar did)."""
    if planar is None and (frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3):
        raise ValueError(f"with size set, frames must be [F,h,w,3] uint8 (the reference resizes 8-bit images), got {tuple(frames.shape)} {frames.dtype}")
    try:
        hh, ww = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    if hh < 1 or ww < 1:
        raise ValueError(f"size must be positive, got {size!r}")
    return hh, ww


def _source(frames, size, crop, resample, pixel_format, yuv_matrix, yuv_range):
    """What the two clip entry points make of (frames, size, crop, resample, pixel_format, ...), validated before anything runs:
    (u8_in, hh, ww, shrink) -- whether chunks reach the routes as uint8 [n,H,W,3], the model grid, and the device-side step from an
    uploaded chunk to the routes' frames (nothing, the conversion, the resize or the resize that converts)."""
    from . import ops
    planar = _planar(frames, pixel_format, yuv_matrix, yuv_range)
    u8_in = frames.dtype == torch.uint8
    if planar is None and (frames.dim() != 4 or frames.shape[-1 if u8_in else 1] != 3 or not (u8_in or frames.dtype == torch.float32)):
        raise ValueError(f"frames must be [F,3,H,W] float32 or [F,H,W,3] uint8, got {tuple(frames.shape)} {frames.dtype}")
    fh, fw = planar if planar is not None else (frames.shape[1:3] if u8_in else frames.shape[2:4])
    kw = {} if planar is None else {"pixel_format": pixel_format, "yuv_matrix": yuv_matrix, "yuv_range": yuv_range}
    if size is None:
        shrink = (lambda chunk: chunk) if planar is None else (lambda chunk: yuv420_to_rgb(chunk, **kw))
        return u8_in, fh, fw, shrink
    hh, ww = _sized(frames, size, planar)
    box = reference_crop(crop, fh, fw) if isinstance(crop, str) else crop
    ops._resize_filter(resample)                                                   # bad resample / crop: before anything runs
    if frames.shape[0]:
        ops._resize_args((frames.shape[0], fh, fw, 3), (hh, ww), box)
    return u8_in, hh, ww, lambda chunk: resize_frames(chunk, (hh, ww), box, resample, **kw)


_UPLOAD_STREAMS = {}         # device index -> the module's one side stream for uploads


def _chunks(fn, frames: torch.Tensor, per_call: int, dev):
    """The chunks frames[f0 : f0 + per_call] on `dev`, in order; records the route in fn.last_upload.
    'overlapped' (host frames in pinned memory, a GPU model): chunk k + 1 is copied with non_blocking=True on the module's side stream
    of that device while the caller's stream computes on chunk k.  The copy waits for what the compute stream held when it was issued
    (chunk k - 1's work), the compute stream waits for the copy's event before it touches the chunk, and record_stream keeps the
    chunk's memory from reuse while that work runs.  The caller drops chunk k before asking for k + 1: at most two are resident.
    Before the generator ends -- exhausted, or closed by an exception in the caller -- the host waits for the side stream: copies
    complete in order, so every copy out of `frames` is done and the caller may overwrite its buffer as soon as the clip call returns,
    as with the blocking copies.  (The last chunk's compute is enqueued by then: the wait hides nothing from the device.)
    'sync' (anything else): frames[...].to(dev) per chunk, as before."""
    dev = torch.device(dev)
    n_frames = frames.shape[0]
    overlapped = dev.type == "cuda" and not frames.is_cuda and frames.is_pinned()
    fn.last_upload = "overlapped" if overlapped else "sync"
    if not overlapped:
        for f0 in range(0, n_frames, per_call):
            yield frames[f0:f0 + per_call].to(dev)
        return
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    side = _UPLOAD_STREAMS.get(index)
    if side is None:
        side = _UPLOAD_STREAMS[index] = torch.cuda.Stream(device=index)
    compute = torch.cuda.current_stream(index)

    def start(f0):
        side.wait_stream(compute)
        with torch.cuda.stream(side):
            chunk = frames[f0:f0 + per_call].to(dev, non_blocking=True)
            return chunk, side.record_event()

    try:
        ahead = start(0) if n_frames else None
        for f0 in range(0, n_frames, per_call):
            chunk, ready = ahead
            ahead = start(f0 + per_call) if f0 + per_call < n_frames else None
            compute.wait_event(ready)
            chunk.record_stream(compute)
            yield chunk
            del chunk
    finally:
        side.synchronize()           # no copy out of the caller's buffer is in flight once the call returns


def _check_out(out, n_images: int, spec):
    """out= of the clip calls: None, or a contiguous tensor of exactly the images' shape and dtype (ValueError otherwise)."""
    if out is None:
        return
    want = (n_images,) + spec.shape
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.dtype != spec.out_dtype or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {spec.out_dtype} tensor {want} (the images of this call), got "
                         f"{tuple(out.shape) if isinstance(out, torch.Tensor) else type(out)} {getattr(out, 'dtype', '')}")


_DOWNLOAD_STREAMS = {}       # device index -> the module's one side stream for downloads


class _Downloads:
    """The way out of a clip call with out=: the mirror image of _chunks.  Records the route in fn.last_download.
    'overlapped' (out in pinned host memory, a GPU model): the images of chunk k are written to one of two device staging buffers
    (staging), then copied with non_blocking=True into out[...] on the module's download stream of that device while the caller's stream
    computes chunk k + 1 (put).  The copy waits for an event recorded after the chunk's emit; the compute stream waits for a staging
    buffer's last copy before it writes the buffer again.  finish() makes the host wait for the side stream -- the clip calls run it in a
    finally, so also when an exception unwinds --: every byte of `out` is valid when the call returns.
    'sync' (pageable or device `out`, a CPU model): out[...].copy_(images) per chunk."""

    def __init__(self, fn, out, shape, per_chunk: int, dev):
        dev = torch.device(dev)
        self.out, self.pos, self.shape, self.per_chunk = out, 0, tuple(shape), per_chunk
        self.overlapped = dev.type == "cuda" and not out.is_cuda and out.is_pinned()
        fn.last_download = "overlapped" if self.overlapped else "sync"
        if self.overlapped:
            self.index = dev.index if dev.index is not None else torch.cuda.current_device()
            self.side = _DOWNLOAD_STREAMS.get(self.index)
            if self.side is None:
                self.side = _DOWNLOAD_STREAMS[self.index] = torch.cuda.Stream(device=self.index)
            self.compute = torch.cuda.current_stream(self.index)
            self.bufs, self.done, self.turn = [None, None], [None, None], 0

    def staging(self, n: int):
        """The device tensor [n, 1, *shape] the next chunk's images go to, or None (sync: the producer allocates as it always did)."""
        if not self.overlapped:
            return None
        i = self.turn
        if self.bufs[i] is None:
            with torch.cuda.device(self.index):
                self.bufs[i] = torch.empty((self.per_chunk, 1) + self.shape, dtype=self.out.dtype, device=f"cuda:{self.index}")
        if self.done[i] is not None:
            self.compute.wait_event(self.done[i])          # the buffer's last copy has left it
        return self.bufs[i][:n]

    def put(self, imgs: torch.Tensor):
        """imgs [n, *shape]: the chunk just produced (staging's buffer when overlapped) -> out[pos : pos + n]."""
        n = imgs.shape[0]
        dst = self.out[self.pos:self.pos + n]
        self.pos += n
        if not self.overlapped:
            dst.copy_(imgs)
            return
        self.side.wait_event(self.compute.record_event())   # the chunk's emit
        with torch.cuda.stream(self.side):
            dst.copy_(imgs, non_blocking=True)
            self.done[self.turn] = self.side.record_event()
        self.turn ^= 1

    def finish(self):
        if self.overlapped:
            self.side.synchronize()


class _Route:
    """What differs between the clip calls: a route takes the chunks of _run_clip in order and carries the state `h`.  fused: run(ci,
    chunk, buf) makes the images [n * k, *spec.shape] of chunk ci ([n,3,H,W] float32 or [n,H,W,3] uint8) in one driver call, in `buf`
    [n * k, 1, *spec.shape] when there is one.  Otherwise (the Python loops) run(ci, chunk, buf) yields them one by one as float32
    [1,c,H,W] in [0, 1]; _run_clip gives them the call's dtype and format."""
    fused = False

    def __init__(self, model, h: torch.Tensor, k: int, step_n: int):
        self.model, self.h, self.k, self.step_n = model, h, k, step_n


def _loop_image(img: torch.Tensor, spec) -> torch.Tensor:
    """A loop route's image as the call's: float32 as it is, or truncated to uint8 [1,H,W,c] and from there to planar YUV."""
    if spec.out_dtype == torch.uint8:
        img = (img * 255.0).to(torch.uint8).permute(0, 2, 3, 1)
    return rgb_to_yuv420(img.contiguous(), spec.out_format, spec.yuv_matrix, spec.yuv_range) if spec.planar else img


class _Delivery:
    """out_size= of the clip calls: the step between the route and the sink.  The routes run at the model grid and make uint8 RGB24
    images there exactly as without out_size; enlarge() turns a chunk's grid images [n,H,W,3] into the images of
    the call (spec: their ImageSpec, at the delivery size) -- 'rgb24' by ncahip_clip_resize_u8, 'i420' / 'nv12' by
    ncahip_clip_resize_u8_yuv420 (no full-size RGB image), CPU images by the numpy mirrors -- the whole grid image, no crop."""

    def __init__(self, spec, resample: str):
        self.spec, self.resample = spec, resample

    def enlarge(self, imgs: torch.Tensor, into: Optional[torch.Tensor]) -> torch.Tensor:
        """imgs [n,H,W,3] uint8 -> [n, *spec.shape], written to `into` (a device tensor of that shape) when there is one."""
        from . import ops
        s, size = self.spec, (self.spec.H, self.spec.W)
        if not imgs.is_cuda:
            big = resize_frames(imgs, size, None, self.resample, out_format=s.out_format, out_yuv_matrix=s.yuv_matrix, out_yuv_range=s.yuv_range)
            return big if into is None else into.copy_(big)
        if s.planar:
            return ops.clip_resize_to_yuv420(imgs, size, None, self.resample, s.out_format, s.yuv_matrix, s.yuv_range, out=into)
        return ops.clip_resize(imgs, size, None, self.resample, out=into)


def _image_specs(out_size, out_resample, out_dtype, out_format, out_yuv_matrix, out_yuv_range, c_out: int, hh: int, ww: int):
    """(spec, deliver) of a clip call, validated before anything runs: the ImageSpec the routes emit with, and None or the _Delivery of
    out_size=(h, w).  With out_size the routes emit uint8 RGB24 at the grid, and every rule of the images -- the dtype, c_out == 3, the
    even sides of a planar format -- applies to the delivery size."""
    from . import ops
    if out_size is None:
        return ops.ImageSpec.of(out_dtype, out_format, out_yuv_matrix, out_yuv_range, c_out, hh, ww), None
    if out_dtype != torch.uint8:
        raise ValueError(f"out_size needs out_dtype=torch.uint8 (Pillow's resize is an 8-bit algorithm, as on the way in), got {out_dtype}")
    try:
        oh, ow = (operator.index(v) for v in out_size)               # integers only: 36.5 is not truncated to 36
    except (TypeError, ValueError):
        raise ValueError(f"out_size must be (h, w), two integers, got {out_size!r}") from None
    if oh < 1 or ow < 1:
        raise ValueError(f"out_size must be positive, got {out_size!r}")
    if out_resample not in ("bicubic", "lanczos"):
        raise ValueError(f"out_resample must be 'bicubic' or 'lanczos', got {out_resample!r}")
    if c_out != 3:
        raise ValueError(f"out_size needs an RGB image (c_out == 3), got c_out = {c_out}")
    spec = ops.ImageSpec.of(out_dtype, out_format, out_yuv_matrix, out_yuv_range, c_out, oh, ow)      # (planar: even out_size)
    ops._resize_args((1, hh, ww, 3), (oh, ow), None)
    return ops.ImageSpec.of(torch.uint8, "rgb24", c_out=c_out, H=hh, W=ww), _Delivery(spec, out_resample)


def _run_clip(fn, route: _Route, frames: torch.Tensor, shrink, per_call: int, dev, spec, out, deliver: Optional[_Delivery] = None):
    """The chunk pipeline of both clip calls (fn: the entry point, which records the routes taken), returning (images, state).  Per chunk
    of per_call frames: upload (_chunks), shrink, the staging buffer of out= (_Downloads), the route, with out_size= the enlargement of
    the chunk's images (deliver: the staging buffer then has the delivery shape and receives the enlarged images), the images on their way
    to `out` or to the final cat.  raw and chunk are dropped before the next chunk is asked for (_chunks: at most two uploaded chunks
    alive).  spec: what the route emits; the images of the call are deliver.spec's when there is a deliver."""
    k = route.k
    fn.last_path, fn.last_download = "clip" if route.fused else "loop", None
    out_spec = spec if deliver is None else deliver.spec
    sink = None if out is None else _Downloads(fn, out, out_spec.shape, per_call * k, dev)
    outs = []
    try:
        for ci, raw in enumerate(_chunks(fn, frames, per_call, dev)):
            chunk = shrink(raw)
            buf = None if sink is None else sink.staging(chunk.shape[0] * k)
            if deliver is not None:                        # the route as without out_size, then the step to the delivery size
                imgs = [route.run(ci, chunk, None)] if route.fused else [_loop_image(img, spec) for img in route.run(ci, chunk, None)]
                if imgs:
                    grid = imgs[0] if len(imgs) == 1 else torch.cat(imgs)     # (a fused route's one tensor is not copied)
                    imgs = [deliver.enlarge(grid.contiguous(), None if buf is None else buf[:, 0])]
            elif route.fused:
                imgs = [route.run(ci, chunk, buf)]
            else:
                imgs = [_loop_image(img, spec) for img in route.run(ci, chunk, buf)]
                if sink is not None and imgs:              # one tensor per chunk, in the staging buffer when there is one
                    imgs = [torch.cat(imgs) if buf is None else buf[:, 0].copy_(torch.cat(imgs))]
            if sink is None:
                outs.extend(imgs)
            elif imgs:
                sink.put(imgs[0])
            del raw, chunk                                 # (_chunks: at most two uploaded chunks alive)
    finally:
        if sink is not None:
            sink.finish()                # no copy into the caller's buffer is in flight once the call returns
    fn.last_state = route.h
    if sink is not None:
        return out, route.h
    return (torch.cat(outs) if outs else torch.empty((0,) + out_spec.shape, dtype=out_spec.out_dtype, device=dev)), route.h


def _check_precision(nca_model, h: torch.Tensor, precision: str, direction) -> None:
    """stylize_clip(precision='bf16' / 'bf16_wide'): ValueError unless the model, its steps and the state run in that arithmetic."""
    from . import ops
    if precision == "f32":
        return
    fc = nca_model.w1.out_channels
    if precision == "bf16" and not ops.dynca_bf16_ok(nca_model.c_in, fc):
        raise ValueError(f"precision='bf16' covers C <= 16 and fc <= 128 (ops.dynca_bf16_ok); the model has C = {nca_model.c_in}, fc = {fc}")
    if precision == "bf16_wide" and not ops.dynca_bf16_wide_ok(nca_model.c_in, fc):
        raise ValueError(f"precision='bf16_wide' covers C <= 32 and fc <= 256 (ops.dynca_bf16_wide_ok); the model has C = {nca_model.c_in}, fc = {fc}")
    if not ops.dynca_bf16_ok(nca_model.c_in, fc):
        # 'bf16_wide' beyond the narrow range: the single-scale unsteered step only, whatever the state is
        if nca_model._multiscale():
            raise ValueError(f"precision='bf16_wide' needs the fused step kernels; multi-scale perception at C = {nca_model.c_in}, fc = {fc} "
                             "runs the composed multi-scale step")
        if direction is not None:
            raise ValueError(f"precision='bf16_wide' does not steer beyond C <= 16 and fc <= 128 (ops.dynca_bf16_ok): a direction on a model "
                             f"with C = {nca_model.c_in}, fc = {fc} would run in fp32")
    if not h.is_cuda or h.dtype != torch.float32:
        raise ValueError(f"precision={precision!r} needs a float32 state on the GPU (the state stays fp32), got {h.dtype} on {h.device}")
    if nca_model._composed(h):
        raise ValueError(f"precision={precision!r} needs the fused step kernels; this model's perception scales / size run the composed multi-scale step")


class _DyncaClip(_Route):
    """stylize_clip's clip route, edge-conditioned and extra-channel models: per call the weights, the filter bank or the positional
    encoding (turned by `angle`, as forward_nsteps turns it) and two_scale; per chunk ncahip_clip_cond / ncahip_clip_gray, the loop's own
    mask draws call by call (DyNCA._draw: the generator ends where it would) and one driver call."""
    fused = True

    def __init__(self, model, h, k, step_n, gray, angle, spec):
        from . import ops, steer
        super().__init__(model, h, k, step_n)
        self.gray, self.size, self.okw = gray, (spec.H, spec.W), spec.keywords
        self.w = ops.DyncaWeights(model.w1.weight, model.w1.bias, model.w2.weight, model.w2.bias, h)
        self.two, self.extra = list(model.perception_scales) == [0, 1], _extra_channels(model)
        if self.extra:
            self.pos = model._cond(h.new_empty(1, model.c_in, *self.size))       # CPE (or None): a function of the shape alone
            if self.pos is not None and angle is not None:
                self.pos = steer.rotate_pos_emb(self.pos, angle)
        else:
            layer = model.cond_layer
            self.bank = torch.cat((layer.sobel_x.weight, layer.sobel_y.weight, layer.laplacian.weight), dim=0)
            self.do_tanh = isinstance(layer.edge_transform, torch.nn.Tanh)

    def run(self, ci, chunk, buf):
        from . import ops
        m, k, step_n, rate = self.model, self.k, self.step_n, 0.5
        chunk = chunk.unsqueeze(1)                                                # [n,1,3,H,W] or [n,1,H,W,3]
        calls = chunk.shape[0] * k
        cond = ops.clip_gray(chunk, self.gray) if self.extra else ops.clip_cond(chunk, self.bank, self.gray, self.do_tanh)
        us = None
        if m.mask_rng != "philox":
            us = torch.cat([ops.draw_fire_masks(1, *self.size, step_n, rate, "dynca", self.h.device) for _ in range(calls)])
        args = (us, self.w, k, step_n, m.c_out, m.padding_mode, rate, m.mask_seed, m._mask_step)
        if self.extra:                             # h keeps c_in - 1 channels: the driver's last channel is the grey frame
            imgs, x = ops.dynca_clip_xc(self.h, cond, self.pos, *args, two_scale=self.two, images=buf, **self.okw)
            self.h = x[:, :-1]
        else:
            imgs, self.h = ops.dynca_clip(self.h, cond, *args, two_scale=self.two, images=buf, **self.okw)
        m._mask_step += calls * step_n
        return imgs[:, 0]


class _DyncaLoop(_Route):
    """stylize_clip's Python loop over forward_nsteps; `direction` goes to forward_nsteps, which attaches it per call."""

    def __init__(self, model, h, k, step_n, gray, direction, u8_in):
        super().__init__(model, h, k, step_n)
        self.gray, self.u8_in, self.extra = gray, u8_in, _extra_channels(model)
        self.steer_kw = {} if direction is None else {"direction": direction}     # (a model without the keyword still runs unsteered clips)

    def run(self, ci, chunk, buf):
        m = self.model
        chunk = _widen(chunk) if self.u8_in else chunk
        for i in range(chunk.shape[0]):
            cond = _gray(chunk[i:i + 1], self.gray)
            for _ in range(self.k):
                if self.extra:      # the grey frame as the last state channel, dropped again after the call
                    x, rgb = m.forward_nsteps(torch.cat((self.h, cond.to(self.h.dtype)), 1), self.step_n, **self.steer_kw)
                    self.h = x[:, :-1]
                else:
                    self.h, rgb = m.forward_nsteps(self.h, self.step_n, cond_img=cond, **self.steer_kw)
                yield (rgb.float().clamp(-1.0, 1.0) + 1.0) / 2.0


@torch.no_grad()
def stylize_clip(nca_model, frames: torch.Tensor, step_n: int = 8, steps_per_frame: int = 1, state: Optional[torch.Tensor] = None,
                 gray: str = "mean", out_dtype=torch.float32, frames_per_call: int = 32, size=None, crop="dynca", resample: str = "bicubic",
                 precision: str = "f32", direction=None, pixel_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited",
                 out_format: str = "rgb24", out_yuv_matrix: str = "bt709", out_yuv_range: str = "limited", out: Optional[torch.Tensor] = None,
                 out_size=None, out_resample: str = "bicubic"):
    """A whole clip per call: video_utils.py:50-83 over `frames`, returning (images, state).

    frames: [F,3,H,W] float32 in [-1, 1] or [F,H,W,3] uint8 (what a decoder delivers), on the host or the device.  images:
    [F*steps_per_frame,3,H,W] float32 in [0, 1], or [F*steps_per_frame,H,W,3] uint8 (truncated, as VideoWriter.add) with
    out_dtype=torch.uint8, on the model's device.  state: None seeds as synthesize_video does; pass the returned state to continue.
    gray: 'mean' (the reference's RGBToGrayscale, the default) or 'luma' (what synthesize_video conditions on).

    Models with edge conditioning and perception_scales [0] or the fused [0, 1] run frames_per_call frames per C call
    (ncahip_clip_cond, then ncahip_dynca_clip_f32: the library's step kernels and the image output, no Python per frame); the result
    does not depend on frames_per_call.  The fire masks follow the model's mask_rng exactly as forward_nsteps draws them.  Anything else
    (other conditioning or scale sets, non-fp32 state, CPU tensors) runs a Python loop over forward_nsteps with the chosen grey.
    stylize_clip.last_path records the route: 'clip' or 'loop'.

    Extra-channel models (ncahip.models.dynca_extra.DyNCA; ExtraChannels/utils/misc/video_utils.py:66-82): per (frame, k) the grey frame
    becomes the last state channel, forward_nsteps runs, the channel is dropped again.  `state` in and out is the reference's `h` with
    c_in - 1 channels (anything else: ValueError).  perception_scales [0] or the fused [0, 1] with an fp32 state run frames_per_call
    frames per C call (ncahip_clip_gray, then ncahip_dynca_clip_xc_f32 with the model's positional encoding); anything else runs that
    loop in Python.

    size=(H, W): decoder-sized frames.  frames must then be uint8 [F,h,w,3] (float frames: ValueError -- the reference resizes 8-bit
    images); every chunk is uploaded at its native size, shrunk on the device by resize_frames(chunk, size, crop, resample) -- the
    reference's preprocess_style_image (crop='dynca', bicubic), bit for bit -- and handed to the uint8 path above unchanged, on both
    routes.  Seeding, the state and the images use (H, W).  size=None: crop and resample are not looked at.

    precision: 'f32' (exact, the default), 'bf16' or 'bf16_wide' -- the steps of this call run under ops.dynca_precision(precision)
    (both 1x1 products on bf16 MFMA, fp32 accumulation and state; include/ncahip.h, ncahip_dynca_precision and
    ncahip_dynca_bf16_range), on both routes and for both model families; the process-wide mode is afterwards what it was before.
    'bf16' needs ops.dynca_bf16_ok(c_in, fc_dim), 'bf16_wide' ops.dynca_bf16_wide_ok(c_in, fc_dim) (C <= 32, fc <= 256); both need an
    fp32 state on the GPU and a model whose steps run on the fused kernels, and a `direction` needs a model inside dynca_bf16_ok:
    anything else raises ValueError rather than computing in the other arithmetic.

    direction: None, a field tensor [1,2,H,W] or an (alignment, angle_deg) tuple (ncahip.steer; forward_nsteps' keyword): every step of
    the call rotates each cell's Sobel pair by its direction -- 'flow to the left', 'outwards from the centre', 'round two poles' for a
    trained motion model.  ONE field serves the whole call (no field per frame), on both routes and for both model families; with a
    tuple, an extra-channel model's positional encoding is turned by the angle as well.  Needs an fp32 state.

    pixel_format: 'rgb24' (the default: frames as described above) or 'i420' / 'nv12' -- frames are planar YUV 4:2:0 [F, 3h/2, w] uint8 as
    the decoder wrote them (yuv420_to_rgb; yuv_matrix 'bt601' / 'bt709', yuv_range 'limited' / 'full'; any other shape or dtype, odd h or
    w: ValueError).  Every chunk is uploaded as it is (1.5 bytes per pixel) and becomes RGB on the device: with size set inside the
    resize (resize_frames(chunk, ..., pixel_format=...)), without it by yuv420_to_rgb; the uint8 path above follows unchanged, on both
    routes and for both model families.  The result is that of the same call on yuv420_to_rgb(frames, ...).

    Uploads: host frames in pinned memory (frames.is_pinned()) with a model on the GPU are uploaded on a side stream, chunk k + 1 while
    chunk k computes; anything else is uploaded as before.  stylize_clip.last_upload records which: 'overlapped' or 'sync'.  Either
    way every copy out of `frames` is complete when the call returns: the caller may overwrite the buffer at once.

    out_format: 'rgb24' (the default: images as described above) or 'i420' / 'nv12' -- images are planar YUV 4:2:0
    [F*steps_per_frame, 3H/2, W] uint8, what a video encoder takes (rgb_to_yuv420; out_yuv_matrix 'bt601' / 'bt709', out_yuv_range
    'limited' / 'full').  Needs out_dtype=torch.uint8, c_out == 3 and even H, W (ValueError otherwise, before any work).  The clip route's
    image output writes the planes straight from the state; the loop route converts its uint8 image.  Either way the result is
    rgb_to_yuv420 of the uint8 images of the same call, bit for bit.

    out: None, or a tensor of exactly the images' shape and dtype (anything else: ValueError before any work) that receives the images
    and is returned as `images`.  A pinned host tensor with a model on the GPU is filled on a side stream, chunk k while chunk k + 1
    computes; the host waits for the last copy before the call returns (also when it raises), so every byte is valid then.  A pageable or
    device tensor is filled by a plain copy per chunk.  stylize_clip.last_download records 'overlapped', 'sync' or None (out=None).

    out_size=(h, w): images at delivery size.  The call runs at the model grid exactly as without it -- the same routes, state and mask
    stream -- and every chunk's uint8 RGB24 images are enlarged on the device between the route and `out`: Pillow's 8-bit Image.resize of
    the whole grid image (out_resample 'bicubic' or 'lanczos'), for 'rgb24' by ncahip_clip_resize_u8, for 'i420' / 'nv12' by
    ncahip_clip_resize_u8_yuv420, whose vertical pass writes the planes (no full-size RGB image).  images: [F*steps_per_frame, h, w, 3] or
    [F*steps_per_frame, 3h/2, w] uint8; `out` and its staging buffers have that shape.  Bit for bit resize_frames(images of the same call
    without out_size, out_size, None, out_resample), and rgb_to_yuv420 of that for a planar format; independent of frames_per_call.  Needs
    out_dtype=torch.uint8 and c_out == 3; a planar format needs an even out_size (the grid may then be odd).  ValueError before any work
    for anything else.  out_size=None: out_resample is not looked at."""
    from . import ops, steer
    if precision not in ("f32", "bf16", "bf16_wide"):
        raise ValueError(f"precision must be 'f32', 'bf16' or 'bf16_wide', got {precision!r}")
    if gray not in ops.GRAY_WEIGHTS:
        raise ValueError(f"gray must be 'mean' or 'luma', got {gray!r}")
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
    u8_in, hh, ww, shrink = _source(frames, size, crop, resample, pixel_format, yuv_matrix, yuv_range)
    k, step_n, per_call = int(steps_per_frame), int(step_n), max(1, int(frames_per_call))
    dev = nca_model.device
    spec, deliver = _image_specs(out_size, out_resample, out_dtype, out_format, out_yuv_matrix, out_yuv_range, getattr(nca_model, "c_out", 3), hh, ww)
    _check_out(out, frames.shape[0] * k, spec if deliver is None else deliver.spec)
    if _extra_channels(nca_model) and state is not None and (state.dim() != 4 or state.shape[1] != nca_model.c_in - 1):
        raise ValueError(f"state must have c_in - 1 = {nca_model.c_in - 1} channels (the grey frame is appended per call), got {tuple(state.shape)}")
    h = state if state is not None else nca_model.seed(1, size=(ww, hh))
    fused = _clip_route(nca_model, h) and torch.device(dev).type == "cuda"
    _check_precision(nca_model, h, precision, direction)
    dirs = angle = None
    if direction is not None:
        if h.dtype != torch.float32:
            raise ValueError(f"direction needs a float32 state (the bf16-storage steps do not steer), got {h.dtype}")
        dirs, angle = steer.resolve(direction, hh, ww, h.device)           # one field for the whole call
        if dirs.shape[0] != 1:
            raise ValueError(f"direction field must be [1,2,{hh},{ww}] (the clip runs one sample), got {tuple(dirs.shape)}")
    with ops.dynca_precision(precision) if precision != "f32" else contextlib.nullcontext():
        # the clip route's steps run under the field; the loop route hands it to forward_nsteps, which attaches it per call
        with ops.dynca_direction(dirs) if (fused and dirs is not None) else contextlib.nullcontext():
            route = (_DyncaClip(nca_model, h, k, step_n, gray, angle, spec) if fused else
                     _DyncaLoop(nca_model, h, k, step_n, gray, direction, u8_in))
            return _run_clip(stylize_clip, route, frames, shrink, per_call, dev, spec, out, deliver)


stylize_clip.last_path = None
stylize_clip.last_upload = None
stylize_clip.last_download = None


class _CondClip(_Route):
    """stylize_clip_conditioned's clip route: per chunk ncahip_clip_encode, on chunk 0 the warm-up grow with goal[0], the loop's own mask
    draws grow call by grow call (ConditionedNCA._draw: the generator ends where it would) and one driver call.  The state's dtype picks
    the arithmetic: a bfloat16 `h` (precision='bf16') gets a bfloat16 goal and the bf16-storage steps (ncahip_cond_clip_bf16)."""
    fused = True

    def __init__(self, nca, h, k, step_n, warm, spec):
        super().__init__(nca, h.contiguous(), k, step_n)
        self.warm, self.okw, self.w = warm, spec.keywords, nca._weights(self.h)
        self.args = (nca._alive_ch(), nca.alpha_living_threshold, nca.cell_fire_rate, -10.0, 10.0)

    def run(self, ci, chunk, buf):
        from . import ops
        nca, k, step_n, warm = self.model, self.k, self.step_n, self.warm
        draw = lambda steps: None if nca.mask_rng == "philox" else nca._draw(self.h, steps)      # noqa: E731
        chunk = chunk.unsqueeze(1)                                                # [n,1,3,H,W] or [n,1,H,W,3]
        calls = chunk.shape[0] * k
        goal = ops.clip_encode(chunk, nca.encoder, dtype=self.h.dtype)
        if ci == 0 and warm > 0:
            self.h, _, _ = ops.cond_grow(self.h, warm, goal[0], draw(warm), self.w, *self.args, nca.mask_seed, nca._mask_step)
            nca._mask_step += warm
        us = None if nca.mask_rng == "philox" else torch.cat([draw(step_n) for _ in range(calls)])
        imgs, self.h = ops.cond_clip(self.h, goal, us, self.w, k, step_n, *self.args, nca.mask_seed, nca._mask_step, images=buf, **self.okw)
        nca._mask_step += calls * step_n
        return imgs[:, 0]


class _CondLoop(_Route):
    """stylize_clip_conditioned's Python loop over nca.grow, with the warm-up grow before the first frame's steps."""

    def __init__(self, nca, h, k, step_n, warm, u8_in):
        super().__init__(nca, h, k, step_n)
        self.warm, self.u8_in = warm, u8_in

    def run(self, ci, chunk, buf):
        nca = self.model
        if self.u8_in:      # frames as the module takes them: [n,3,H,W] float32 in [0, 1]
            chunk = (chunk.float() / 255.0).permute(0, 3, 1, 2).contiguous()
        for i in range(chunk.shape[0]):
            goal_img = chunk[i:i + 1]
            if ci == 0 and i == 0 and self.warm > 0:
                self.h = nca.grow(self.h, self.warm, goal_img)
            for _ in range(self.k):
                self.h = nca.grow(self.h, self.step_n, goal_img)
                yield torch.clamp(self.h[:, :3].float(), 0.0, 1.0)               # (trainer.py:36-39, utils/utils.py:34-35)


@torch.no_grad()
def stylize_clip_conditioned(nca, frames: torch.Tensor, step_n: int = 8, steps_per_frame: int = 1, state: Optional[torch.Tensor] = None,
                             warmup_steps: int = 0, out_dtype=torch.float32, frames_per_call: int = 8, size=None, crop="conditioned",
                             resample: str = "lanczos", precision: str = "f32", pixel_format: str = "rgb24", yuv_matrix: str = "bt709",
                             yuv_range: str = "limited", out_format: str = "rgb24", out_yuv_matrix: str = "bt709", out_yuv_range: str = "limited",
                             out: Optional[torch.Tensor] = None, out_size=None, out_resample: str = "bicubic"):
    """A whole clip per call for a ConditionedNCA (ncahip.nca.ConditionedNCA), returning (images, state): what the reference's interactive
    loop does when the goal is switched while it runs (EncoderConditioning/visualisation.ipynb) -- the state is carried, every frame is the
    goal of its own steps:

        for frame in frames, steps_per_frame times:  state = nca.grow(state, step_n, frame[None]);  image = clamp(state[:, :3], 0, 1)

    frames: [F,3,H,W] float32 in [0, 1] (ToTensor output) or [F,H,W,3] uint8, on the host or the device.  images:
    [F*steps_per_frame,3,H,W] float32 in [0, 1], or [F*steps_per_frame,H,W,3] uint8 (truncated) with out_dtype=torch.uint8, on the model's
    device.  state: None starts from nca.generate_seed(1, size=H) (H == W required then); pass the returned state to continue.
    warmup_steps: extra steps on frame 0's goal before the first image (a seed needs tens of steps to grow).

    An fp32 state on the GPU with one sample and an ImageEncoder the fused kernel covers run frames_per_call frames per C call
    (ncahip_clip_encode for the goals of the chunk -- 34 MB at 8 x 256^2, E = 16 --, then ncahip_cond_clip_f32: the library's grow drivers and
    the image output, no Python per frame); the result does not depend on frames_per_call.  The fire masks are drawn exactly as
    ConditionedNCA._draw draws them per grow call, in order, and _mask_step advances as in the loop.  Anything else (a custom encoder, a bf16
    state) runs the loop above in Python.  stylize_clip_conditioned.last_path records the route: 'clip' or 'loop'.

    precision: 'f32' (the default: everything above, a bf16 state included, as it always was) or 'bf16' -- the call runs on a bfloat16
    state with the bf16-storage steps (include/ncahip.h, "bf16 state storage": state and goal travel as bf16, the UpdateNet runs on bf16
    MFMA).  state=None seeds as before and casts the seed (exact: zeros and ones); a float32 state is rounded once at entry; a bfloat16
    state is taken as it is.  The returned state is bfloat16, and passing it back is lossless.  With one sample and an ImageEncoder the
    fused kernel covers, the chunk runs on the clip route: ncahip_clip_encode_bf16 (the fused encoder, its store rounded), the warm-up
    grow, then ncahip_cond_clip_bf16, whose last launch per image resolves the state and writes the image in one pass; otherwise the loop
    above runs on the bfloat16 state.  Mask draws, _mask_step, frames_per_call independence, size=, pixel_format=, out_format= and out=
    work as with 'f32'.  Needs a model on the GPU with num_channels <= 20 and W % 4 == 0 (what the bf16-storage kernels cover): anything
    else raises ValueError before any work rather than computing in the other arithmetic.

    size=(H, W): decoder-sized frames, as in stylize_clip: uint8 [F,h,w,3] frames only (float frames: ValueError), each chunk uploaded at
    its native size and shrunk on the device by resize_frames(chunk, size, crop, resample) -- the reference's load_image (crop='conditioned',
    Lanczos), bit for bit -- on both routes; seeding, the state check and the images use (H, W).  size=None: crop and resample are not
    looked at.

    pixel_format, yuv_matrix, yuv_range: planar YUV 4:2:0 frames [F, 3h/2, w] uint8 ('i420' / 'nv12'), as in stylize_clip: converted on the
    device, inside the resize when size is set; the result is that of the same call on yuv420_to_rgb(frames, ...).  Pinned host frames
    are uploaded on a side stream while the previous chunk computes; stylize_clip_conditioned.last_upload records 'overlapped' or 'sync'.
    Every copy out of `frames` is complete when the call returns.

    out_format, out_yuv_matrix, out_yuv_range, out: planar YUV 4:2:0 images [F*steps_per_frame, 3H/2, W] uint8 and delivery into a
    caller's tensor (a pinned one on a side stream while the next chunk computes), as in stylize_clip;
    stylize_clip_conditioned.last_download records 'overlapped', 'sync' or None.

    out_size, out_resample: images at delivery size [F*steps_per_frame, h, w, 3] or [F*steps_per_frame, 3h/2, w] uint8, as in stylize_clip:
    the call runs at the grid as without it (both routes, 'f32' and 'bf16'), and every chunk's uint8 images are enlarged on the device on
    their way to `out` -- bit for bit resize_frames(images of the same call without out_size, out_size, None, out_resample), and
    rgb_to_yuv420 of that for a planar format.  Needs out_dtype=torch.uint8; a planar format needs an even out_size."""
    from . import ops
    if precision not in ("f32", "bf16"):
        raise ValueError(f"precision must be 'f32' or 'bf16', got {precision!r}")
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"out_dtype must be torch.float32 or torch.uint8, got {out_dtype}")
    u8_in, hh, ww, shrink = _source(frames, size, crop, resample, pixel_format, yuv_matrix, yuv_range)
    spec, deliver = _image_specs(out_size, out_resample, out_dtype, out_format, out_yuv_matrix, out_yuv_range, 3, hh, ww)
    if precision == "bf16":
        if nca.num_channels > 20:
            raise ValueError(f"precision='bf16' covers num_channels <= 20 (the bf16-storage step kernels); the model has {nca.num_channels}")
        if ww % 4:
            raise ValueError(f"precision='bf16' needs W % 4 == 0 (the bf16-storage step kernels), got W = {ww}")
        if next(nca.parameters()).device.type != "cuda":
            raise ValueError(f"precision='bf16' needs a model on the GPU, got {next(nca.parameters()).device}")
    if nca.num_target_channels != 3:
        raise ValueError(f"stylize_clip_conditioned needs an RGB model (num_target_channels == 3), got {nca.num_target_channels}")
    if state is not None and (state.dim() != 4 or state.shape[1] != nca.num_channels or tuple(state.shape[2:]) != (hh, ww)):
        raise ValueError(f"state must be [B,{nca.num_channels},{hh},{ww}] (nca.num_channels channels, the frames' size), got {tuple(state.shape)}")
    if state is None and hh != ww:
        raise ValueError(f"state=None seeds a square grid (generate_seed(1, size=H)): frames are {hh} x {ww}; pass a state")
    k, step_n, warm, per_call = int(steps_per_frame), int(step_n), int(warmup_steps), max(1, int(frames_per_call))
    if k < 1 or step_n < 1 or warm < 0:
        raise ValueError("steps_per_frame and step_n must be positive and warmup_steps non-negative")
    _check_out(out, frames.shape[0] * k, spec if deliver is None else deliver.spec)
    dev = next(nca.parameters()).device
    h = (nca.generate_seed(1, size=hh) if state is None else state).to(dev)
    if precision == "bf16":
        h = h.to(torch.bfloat16)
    fused = (h.is_cuda and h.dtype == (torch.float32 if precision == "f32" else torch.bfloat16) and h.shape[0] == 1 and
             ops.encoder_clip_ok(nca.encoder) and nca.encoder.channels == 3)
    route = _CondClip(nca, h, k, step_n, warm, spec) if fused else _CondLoop(nca, h, k, step_n, warm, u8_in)
    return _run_clip(stylize_clip_conditioned, route, frames, shrink, per_call, dev, spec, out, deliver)


stylize_clip_conditioned.last_path = None
stylize_clip_conditioned.last_upload = None
stylize_clip_conditioned.last_download = None
