"""Tensor-level wrappers over the C ABI: marshal torch CUDA tensors to raw pointers, enqueue on the
current torch stream.  Every function here fails loudly for non-CUDA tensors -- the product path
has no CPU fallback (the CPU restatement lives in oracle/ and is test infrastructure only)."""
import contextlib
import re
import threading
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _capi
from ._capi import PAD_MODES, check, lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.NcaHipError(f"ncahip: `{name}` must be a CUDA (ROCm) tensor -- the NCA hot path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"ncahip: `{name}` must be {dtype}, got {t.dtype}")
    return t.contiguous()


_WS_CACHE = {}


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Scratch for the backward drivers, kept per (device, stream) and grown on demand: the drivers take a caller-owned
    workspace of up to ~0.5 GB (BASELINE configs[2]); allocating it afresh per call costs a torch.empty of that size per
    training step.  Work on one stream is ordered, so consecutive calls may share it."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream())
    ws = _WS_CACHE.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = None
        _WS_CACHE.pop(key, None)
        ws = torch.empty(max(nbytes, 1), device=device, dtype=torch.uint8)
        _WS_CACHE[key] = ws
    return ws


_PERSIST_WS = {}


def _persist_workspace(nbytes: int, device: torch.device, count: int = 1):
    """(workspace, epoch) for ncahip_dynca_nsteps_fwd_persist_f32: a dedicated tensor per (device, stream, size), zeroed when it is
    created and whenever its epoch counter runs out; every call gets the next epoch (the library never clears the workspace: the
    exchanged pairs are tagged epoch * 4096 + step).  count: the number of consecutive epochs the caller will consume, epoch ..
    epoch + count - 1 (ncahip_dynca_clip_f32 uses one per persistent launch)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(), nbytes)
    ent = _PERSIST_WS.get(key)
    if ent is None or ent[1] + count > (1 << 20) - 2:
        ent = [torch.zeros(nbytes, device=device, dtype=torch.uint8), 0]
        _PERSIST_WS[key] = ent
    first = ent[1] + 1
    ent[1] += count
    return ent[0], first


def release_workspaces() -> None:
    """Drop the cached workspaces and the device copies of the resize tables (they are re-created on the next use)."""
    _WS_CACHE.clear()
    _PERSIST_WS.clear()
    _RESIZE_TABLES_DEV.clear()


def _state_dtype(x: torch.Tensor):
    """The fused steps exist for fp32 and for bf16 state storage (ncahip_*_bf16, see include/ncahip.h)."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ncahip: the NCA state must be float32 or bfloat16, got {x.dtype}")
    return x.dtype, ("bf16" if x.dtype == torch.bfloat16 else "f32")


def _w(t: torch.Tensor, name: str, like: torch.Tensor) -> torch.Tensor:
    """weights: detach, squeeze 1x1 conv dims, move next to the state if needed."""
    t = t.detach()
    if t.device != like.device:
        t = t.to(like.device)
    return _dev(t.float(), name)


NO_FUSED_STEPS = 1 << 24        # force_generic bit: the off switch of cond_grow's fused-steps launches
FUSED_STEPS_CAP_SHIFT = 25      # force_generic bits 25-27: steps per fused-steps launch


def force_generic(on) -> None:
    """Test hook (see ncahip.h; the bits are decoded in csrc/nca_modes.hip): True/1 = generic any-shape kernels, 2 = symmetric wave-private ConditionedNCA
    kernel, 32 = fp32 producer/consumer step without firing-cell lists, 64 = firing-cell lists without the carry across
    tiles, 128 = cond_grow's steps draw their fire masks in the kernel (no fire words), n << 8 = at most n workgroups per
    producer/consumer step launch, n << 16 = at most n steps per fire-word launch (and no minimum grow length or grid size),
    NO_FUSED_STEPS (1 << 24) = cond_grow's steps go out one launch each (no fused-steps launches), n << 25 (n <= 7) = at most n steps
    per fused-steps launch, False/0 = defaults."""
    lib().ncahip_debug_force_generic(int(on))


def set_cond_precision(mode) -> None:
    """'exact' / 0 (default) or 'bf16x3' / 1: see ncahip_cond_precision in include/ncahip.h."""
    check(lib().ncahip_cond_precision({"exact": 0, "bf16x3": 1}.get(mode, mode)), "cond_precision")


# the forward's names: (ncahip_dynca_precision mode, ncahip_dynca_bf16_range) pairs
_DYNCA_FWD_PRECISIONS = {"f32": (0, 0), "bf16": (1, 0), "bf16_wide": (1, 1)}
_dynca_precision_lock = threading.RLock()


def set_dynca_precision(mode: str) -> str:
    """'f32' (exact, the default), 'bf16' or 'bf16_wide': both 1x1 products of the DyNCA FORWARD step on bf16 MFMA with fp32
    accumulation -- ncahip_dynca_precision and ncahip_dynca_bf16_range in include/ncahip.h.  'bf16' covers C <= 16 and fc <= 128
    (dynca_bf16_ok); 'bf16_wide' covers those shapes exactly as 'bf16' does and, for single-scale unsteered per-step calls, also
    C <= 32 and fc <= 256 (dynca_bf16_wide_ok).  Other shapes ignore the mode.  Process-wide, read when a call enqueues; needs no GPU.
    Returns the previous name (one of the three).  Whatever keeps a history for autograd runs under 'f32' regardless (the backward
    recomputes exactly)."""
    if mode not in _DYNCA_FWD_PRECISIONS:
        raise ValueError(f"dynca precision must be 'f32', 'bf16' or 'bf16_wide', got {mode!r}")
    prec, rng = _DYNCA_FWD_PRECISIONS[mode]
    with _dynca_precision_lock:
        # two settings, one name: a call enqueued on another thread between the two lines never sees (1, a range nobody asked for) --
        # switching mode 1 on, the range goes first; switching it off, last
        if prec == 1:
            prev_rng = lib().ncahip_dynca_bf16_range(rng)
        prev = lib().ncahip_dynca_precision(prec)
        if prec != 1:
            prev_rng = lib().ncahip_dynca_bf16_range(rng)
        if prev not in (0, 1):
            check(prev, "dynca_precision")
        if prev_rng not in (0, 1):
            check(prev_rng, "dynca_bf16_range")
    # the range matters only while the precision is 1: (0, wide) is not a state this module leaves behind, and reads as 'f32'
    return "f32" if prev == 0 else ("bf16_wide" if prev_rng == 1 else "bf16")


@contextlib.contextmanager
def dynca_precision(mode: str):
    """with ops.dynca_precision('bf16'): ... (or 'bf16_wide', 'f32')  -- set_dynca_precision(mode) for the block, the previous mode back on exit (exceptions
    included).  The mode is process-wide: the block holds a re-entrant lock, so blocks of other threads wait for it."""
    with _dynca_precision_lock:
        prev = set_dynca_precision(mode)
        try:
            yield
        finally:
            set_dynca_precision(prev)


_dynca_direction_lock = threading.RLock()
_dynca_direction_cur = None      # the attached field: the reference that keeps its memory alive while the library holds the pointer


def _attach_direction(dirs: Optional[torch.Tensor]) -> None:
    global _dynca_direction_cur
    if dirs is None:
        check(lib().ncahip_dynca_direction(None, 0, 0, 0), "dynca_direction")
    else:
        check(lib().ncahip_dynca_direction(dirs.data_ptr(), dirs.shape[0], dirs.shape[2], dirs.shape[3]), "dynca_direction")
    _dynca_direction_cur = dirs


@contextlib.contextmanager
def dynca_direction(dirs: torch.Tensor):
    """with ops.dynca_direction(dirs): ...  -- the fused DyNCA forward steps of the block rotate every cell's Sobel pair by its
    direction: dirs [Bd,2,H,W] float32 CUDA contiguous, Bd in {1, B}, plane 0 = s, plane 1 = c; Sx' = c Sx - s Sy, Sy' = s Sx + c Sy
    (ncahip_dynca_direction in include/ncahip.h; ncahip.steer builds fields).  dynca_step, dynca_nsteps (fp32 states), dynca_clip and
    dynca_clip_xc honour it; the backward and the bf16-storage steps refuse to run while it is attached.  The block holds a reference
    to the tensor (the library keeps the pointer, not a copy) and a re-entrant lock, as dynca_precision does; on exit -- exceptions
    included -- the field attached before the block (normally none) is back.  Do not write to dirs while work enqueued in the block
    may still run."""
    if not isinstance(dirs, torch.Tensor) or not dirs.is_cuda:
        raise _capi.NcaHipError("ncahip: the direction field must be a CUDA (ROCm) tensor -- the NCA hot path has no CPU fallback")
    if dirs.dtype != torch.float32:
        raise TypeError(f"ncahip: the direction field must be float32, got {dirs.dtype}")
    if dirs.dim() != 4 or dirs.shape[1] != 2 or not dirs.is_contiguous():
        raise ValueError(f"ncahip: the direction field must be a contiguous [Bd,2,H,W] tensor, got {tuple(dirs.shape)}"
                         f"{'' if dirs.is_contiguous() else ' (not contiguous)'}")
    with _dynca_direction_lock:
        prev = _dynca_direction_cur
        _attach_direction(dirs)
        try:
            yield dirs
        finally:
            _attach_direction(prev)


def reset_modes() -> None:
    """Every process-wide mode back to what a fresh process without environment overrides has: force_generic(0) (every hook bit, the
    fused-steps off switch and its cap included), cond precision
    'exact', DyNCA precision 'f32' (its bf16 range narrow), no direction field attached, no dropped tiles, persistent_steps = True, persistent_cond = False.
    Needs no GPU.  Takes the locks of dynca_precision and dynca_direction; it must not be called inside a block of either (the block
    would put its previous mode back on exit)."""
    global persistent_steps, persistent_cond
    with _dynca_precision_lock, _dynca_direction_lock:
        force_generic(0)
        set_cond_precision("exact")
        set_dynca_precision("f32")
        _attach_direction(None)
        lib().ncahip_debug_persist_drop_tiles(0)
        persistent_steps, persistent_cond = True, False


def dynca_bf16_ok(C: int, fc: int) -> bool:
    """Shapes the 'bf16' DyNCA precision covers: C <= 16 and fc <= 128 (one output tile, one hidden slice)."""
    return 1 <= int(C) <= 16 and 1 <= int(fc) <= 128


def dynca_bf16_wide_ok(C: int, fc: int) -> bool:
    """Shapes the 'bf16_wide' DyNCA precision covers: C <= 32 and fc <= 256 (two output tiles, the whole hidden layer in one launch).
    Beyond dynca_bf16_ok that is the single-scale, unsteered per-step forward only."""
    return 1 <= int(C) <= 32 and 1 <= int(fc) <= 256


def check_errors(clear: bool = True) -> None:
    """Synchronise the current stream and raise NcaHipError if a kernel recorded a device-side failure (a producer/consumer
    hand-off poll that expired) since the last check -- see ncahip_check_errors in include/ncahip.h."""
    rc = lib().ncahip_check_errors(_stream(), int(clear))
    if rc == _capi.EDEVICE:
        msg = (lib().ncahip_last_error() or b"").decode()
        word = re.search(r"error word 0x([0-9a-f]+)", msg)
        if word and int(word.group(1), 16) & 2:      # bit 1: a neighbour poll of a persistent launch expired
            raise _capi.NcaHipError(f"ncahip_check_errors failed (rc={rc}): {msg} -- the persistent grow (ConditionedNCA, "
                                    "ops.persistent_cond = False) and the persistent DyNCA steps (ops.persistent_steps = False) "
                                    "need every tile resident at once; switch them off to run the per-step kernels")
    check(rc, "ncahip_check_errors")


def selftest(device=None) -> None:
    scratch = torch.zeros(1024, dtype=torch.int32, device=device or "cuda")
    check(lib().ncahip_selftest(scratch.data_ptr(), _stream()), "ncahip_selftest")


# ------------------------------------------------------------------------------------ stencils
def dynca_perceive(x: torch.Tensor, pad_mode: str = "replicate") -> torch.Tensor:
    x = _dev(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, 4 * C, H, W, device=x.device, dtype=torch.float32)
    check(lib().ncahip_dynca_perceive_f32(_p(x), _p(y), B, C, H, W, PAD_MODES[pad_mode], _stream()), "dynca_perceive")
    return y


def cond_perceive(z: torch.Tensor, wp: torch.Tensor) -> torch.Tensor:
    z = _dev(z, "z")
    B, C, H, W = z.shape
    wp = _w(wp, "wp", z)
    assert wp.numel() == 27 * C
    y = torch.empty(B, 3 * C, H, W, device=z.device, dtype=torch.float32)
    check(lib().ncahip_cond_perceive_f32(_p(z), _p(wp), _p(y), B, C, H, W, _stream()), "cond_perceive")
    return y


def image_encoder_front(img: torch.Tensor, k3: torch.Tensor, k5: torch.Tensor) -> torch.Tensor:
    """[sobel_x | sobel_y | laplacian](mean over channels) and the per-channel 5x5 blur in one pass (encoder.py:37-52)."""
    img = _dev(img, "img")
    B, ch, H, W = img.shape
    k3, k5 = _w(k3.reshape(-1), "k3", img), _w(k5.reshape(-1), "k5", img)
    assert k3.numel() == 27 and k5.numel() == 25
    feat = torch.empty(B, 3 + ch, H, W, device=img.device, dtype=torch.float32)
    check(lib().ncahip_image_encoder_front_f32(_p(img), _p(k3), _p(k5), _p(feat), B, ch, H, W, _stream()), "image_encoder_front")
    return feat


def edge_extractor(img: torch.Tensor, k3: torch.Tensor, apply_tanh: bool) -> torch.Tensor:
    """[sobel_x | sobel_y | laplacian] of a 1-channel image, zero pad, optional tanh (dynca.py:204-213)."""
    img = _dev(img, "img")
    B, one, H, W = img.shape
    assert one == 1
    k3 = _w(k3.reshape(-1), "k3", img)
    out = torch.empty(B, 3, H, W, device=img.device, dtype=torch.float32)
    check(lib().ncahip_edge_extractor_f32(_p(img), _p(k3), _p(out), B, H, W, int(apply_tanh), _stream()), "edge_extractor")
    return out


# ------------------------------------------------------------------------------------ fire masks as bits
def mask_words(B: int, H: int, W: int) -> int:
    return (B * H * W + 31) // 32


def pack_fire_mask(u: torch.Tensor, rate: float, mode: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u [T,B,1,H,W] float32 draws -> int32 [T, ceil(B*H*W/32)] bit-packed fire masks with the kernels' own predicate
    (mode 'cond': clamp(u,0,1) < rate, nca.py:171-174; 'dynca': floor(u + rate) = 1, dynca.py:131; include/ncahip.h)."""
    u = _dev(u, "u")
    T, B, _, H, W = u.shape
    bits = torch.empty(T, mask_words(B, H, W), device=u.device, dtype=torch.int32) if out is None else out
    assert bits.shape == (T, mask_words(B, H, W)) and bits.dtype == torch.int32 and bits.is_contiguous()
    check(lib().ncahip_pack_fire_mask_u32(_p(u), _p(bits), T, B, H, W, float(rate), {"cond": 0, "dynca": 1}[mode], _stream()),
          "pack_fire_mask")
    return bits


def draw_fire_masks(B: int, H: int, W: int, steps: int, rate: float, mode: str, device, chunk: int = 16) -> torch.Tensor:
    """The reference's per-step uniform draws (nca.py:172 / dynca.py:131: one [B,1,H,W] float32 draw from the device's global
    torch generator per step, nothing in between) evaluated to bit-packed fire masks int32 [steps, ceil(B*H*W/32)].  The
    draws are the same generator calls in the same order as `torch.rand_like(x[:, 0:1])` per step -- `uniform_()` on a
    [B,1,H,W] float32 tensor IS what rand_like runs -- made into a reused chunk buffer (no [T,B,1,H,W] tensor, no stack
    copy) and packed by ncahip_pack_fire_mask_u32 with the kernels' own predicate."""
    bits = torch.empty(steps, mask_words(B, H, W), device=device, dtype=torch.int32)
    buf = torch.empty(min(chunk, steps), B, 1, H, W, device=device, dtype=torch.float32)
    for t0 in range(0, steps, chunk):
        k = min(chunk, steps - t0)
        for j in range(k):
            buf[j].uniform_()
        pack_fire_mask(buf[:k], rate, mode, out=bits[t0:t0 + k])
    return bits


def unpack_fire_mask(bits: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    """int32 [T, words] -> float32 {0,1} masks [T,B,1,H,W] (torch ops; the composed passes and tests)."""
    T = bits.shape[0]
    idx = torch.arange(B * H * W, device=bits.device)
    m = (bits[:, idx >> 5] >> (idx & 31)) & 1
    return m.view(T, B, 1, H, W).float()


def _u_args(us: Optional[torch.Tensor], T: int, B: int, H: int, W: int, seed: int):
    """(tensor, seed) for the C ABI: float32 uniforms [T,B,1,H,W] as they are; int32 bit-packed masks [T, words] with the seed
    that announces them (NCAHIP_SEED_U_IS_BITS); None: in-kernel Philox keyed by `seed`."""
    if us is None:
        return None, seed
    if us.dtype == torch.int32:
        us = _dev(us, "us", torch.int32)
        assert us.numel() == T * mask_words(B, H, W), (tuple(us.shape), T, B, H, W)
        return us, _capi.SEED_U_IS_BITS
    us = _dev(us, "us")
    assert us.numel() == T * B * H * W
    return us, seed


def philox_uniform(B: int, H: int, W: int, seed: int, step: int, device="cuda") -> torch.Tensor:
    u = torch.empty(B, 1, H, W, device=device, dtype=torch.float32)
    check(lib().ncahip_philox_uniform_f32(_p(u), B, H, W, seed, step, _stream()), "philox_uniform")
    return u


def cond_fire_words(Tc: int, B: int, H: int, W: int, fire_rate: float, seed: int, step0: int, device="cuda") -> torch.Tensor:
    """The fire masks of ConditionedNCA steps step0 .. step0 + Tc - 1 (in-kernel Philox) as one 64-bit word per 4 x 16 tile,
    [Tc, B, H/4, W/16] int64: bit 16 * row + col <=> the tile's cell (row, col) fires (ncahip_cond_fire_words)."""
    words = torch.empty(Tc, B, H // 4, W // 16, device=device, dtype=torch.int64)
    check(lib().ncahip_cond_fire_words(_p(words), Tc, B, H, W, fire_rate, seed, step0, _stream()), "cond_fire_words")
    return words


def fire_word_launches() -> int:
    """Test hook: fire-word launches of the last cond_grow on the per-step fp32 kernels (0: its steps drew in the kernel)."""
    return int(lib().ncahip_debug_fire_word_launches())


def fused_step_launches() -> int:
    """Test hook: fused-steps launches (several steps per launch) of the last cond_grow on the fp32 kernels (0: one launch per step)."""
    return int(lib().ncahip_debug_fused_step_launches())


# ------------------------------------------------------------------------------------ DyNCA
class DyncaWeights:
    """w1 [fc,4C+c_cond,1,1], b1 [fc], w2 [C,fc,1,1], b2 [C] as contiguous fp32 device buffers."""

    def __init__(self, w1, b1, w2, b2, like: torch.Tensor):
        self.w1, self.b1 = _w(w1, "w1", like), _w(b1, "b1", like)
        self.w2, self.b2 = _w(w2, "w2", like), _w(b2, "b2", like)
        self.fc, self.k1 = self.w1.shape[0], self.w1.numel() // self.w1.shape[0]
        self.c = self.w2.shape[0]


def dynca_step(x: torch.Tensor, cond: Optional[torch.Tensor], u: Optional[torch.Tensor], w: DyncaWeights,
               pad_mode: str = "replicate", update_rate: float = 0.5, seed: int = 0, step: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    x = _dev(x, "x")
    B, C, H, W = x.shape
    c_cond = 0 if cond is None else cond.shape[1]
    if cond is not None:
        cond = _dev(cond, "cond")
        assert cond.shape == (B, c_cond, H, W)
    if u is not None:
        u = _dev(u, "u")
        assert u.numel() == B * H * W
    assert w.c == C and w.k1 == 4 * C + c_cond, (w.c, w.k1, C, c_cond)
    out = torch.empty_like(x) if out is None else out
    check(lib().ncahip_dynca_step_fwd_f32(_p(x), _p(out), _p(cond), _p(u), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2),
                                          B, C, H, W, w.fc, c_cond, PAD_MODES[pad_mode], update_rate, seed, step,
                                          _stream()), "dynca_step_fwd")
    return out


persistent_steps = True     # dynca_nsteps: use the one-launch persistent kernel where it applies (tests / A-B timing switch it off)
# cond_grow (fp32 state): the whole grow in ONE launch where it applies (ncahip_cond_grow_fwd_persist_f32: the same bits as the
# per-step kernels).  Off by default: at the reference's training shape it only matches the per-step path so far
persistent_cond = False


def two_scale_fused_ok(C: int, H: int, W: int, fc: int, pad_mode: str = "replicate") -> bool:
    """Shapes ncahip_dynca_*_fwd_ms_f32 covers (perception_scales = [0, 1] fused): even sizes, C <= 16, fc <= 128; 'reflect' only
    with a coarse grid of at least 2 x 2 (H, W >= 4: below that F.pad(mode="reflect") raises on the coarse level)."""
    if pad_mode == "reflect" and (H < 4 or W < 4):
        return False
    return H % 2 == 0 and W % 2 == 0 and C <= 16 and fc <= 128


def dynca_nsteps(x: torch.Tensor, T: int, cond: Optional[torch.Tensor], us: Optional[torch.Tensor], w: DyncaWeights,
                 pad_mode: str = "replicate", update_rate: float = 0.5, seed: int = 0, step0: int = 0,
                 keep_history: bool = False, two_scale: bool = False):
    """T fused steps.  Returns (x_T, states) where states is the [ring,B,C,H,W] buffer (ring=T+1 when
    keep_history, else 2).  two_scale: perception_scales = [0, 1] (ncahip_dynca_nsteps_fwd_ms_f32, fp32 states).
    fp32 states honour the ambient dynca_precision, keep_history included (autograd's forward sets 'f32' itself)."""
    dt, sfx = _state_dtype(x)           # bfloat16 state -> bf16-storage entry points (forward only)
    x = _dev(x, "x", dt)
    B, C, H, W = x.shape
    if T == 0:
        return x.clone(), None
    c_cond = 0 if cond is None else cond.shape[1]
    if cond is not None:
        cond = _dev(cond, "cond")
    us, seed = _u_args(us, T, B, H, W, seed)
    assert w.c == C and w.k1 == 4 * C + c_cond, (w.c, w.k1, C, c_cond)
    if not keep_history and sfx == "f32" and persistent_steps and not torch.cuda.is_current_stream_capturing():
        # small grids (B = 1 video inference): all T steps in ONE launch, one workgroup per tile (ncahip_dynca_nsteps_fwd_persist_f32;
        # its epoch is a kernel argument, so never inside a captured graph: no workspace is asked for and no epoch consumed there);
        # NCAHIP_ERANGE = shape not covered or not every tile resident on this device -> the per-step kernels below
        nbytes = lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, w.fc, c_cond)
        if nbytes:
            ws, epoch = _persist_workspace(nbytes, x.device)
            out = torch.empty_like(x)
            fn = lib().ncahip_dynca_nsteps_fwd_persist_ms_f32 if two_scale else lib().ncahip_dynca_nsteps_fwd_persist_f32
            rc = fn(_p(x), _p(out), T, _p(cond), _p(us), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), B, C,
                                                            H, W, w.fc, c_cond, PAD_MODES[pad_mode], update_rate, seed, step0, _p(ws),
                                                            nbytes, epoch, _stream())
            if rc == 0:
                return out, None
            if rc != _capi.ERANGE:
                check(rc, "dynca_nsteps_fwd_persist")
    ring = T + 1 if keep_history else 2
    states = torch.empty(ring, B, C, H, W, device=x.device, dtype=dt)
    states[0].copy_(x)
    if two_scale:
        assert sfx == "f32", "the two-scale step is an fp32 kernel"
        pc = torch.empty(B, 4 * C, H // 2, W // 2, device=x.device, dtype=torch.float32)
        check(lib().ncahip_dynca_nsteps_fwd_ms_f32(_p(states), ring, T, _p(cond), _p(us), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), B, C,
                                                   H, W, w.fc, c_cond, PAD_MODES[pad_mode], update_rate, seed, step0, _p(pc), _stream()),
              "dynca_nsteps_fwd_ms")
        return states[T % ring], states
    check(getattr(lib(), "ncahip_dynca_nsteps_fwd_" + sfx)(_p(states), ring, T, _p(cond), _p(us), _p(w.w1), _p(w.b1), _p(w.w2),
                                                           _p(w.b2), B, C, H, W, w.fc, c_cond, PAD_MODES[pad_mode],
                                                           update_rate, seed, step0, _stream()), "dynca_nsteps_fwd_" + sfx)
    return states[T % ring], states


# ------------------------------------------------------------------------------------ a whole clip per call
GRAY_WEIGHTS = {"mean": (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0),       # the reference's RGBToGrayscale (preprocess_texture.py:178-179)
                "luma": (0.2989, 0.587, 0.114)}                  # ITU-R 601, what ncahip.video.rgb_to_grayscale computes


def _clip_fmt(dtype) -> int:
    if dtype == torch.float32:
        return _capi.CLIP_F32_NCHW
    if dtype == torch.uint8:
        return _capi.CLIP_U8_NHWC
    raise TypeError(f"ncahip: clip frames / images are float32 (channels first) or uint8 (channels last), got {dtype}")


def _frames_dims(frames: torch.Tensor):
    """(fmt, F, B, c, H, W) of clip frames: [F,B,c,H,W] float32 or [F,B,H,W,c] uint8."""
    fmt = _clip_fmt(frames.dtype)
    s = tuple(frames.shape)
    F_, B, c, H, W = s[:2] + s[4:] + s[2:4] if fmt == _capi.CLIP_U8_NHWC else s
    return fmt, F_, B, c, H, W


def clip_cond(frames: torch.Tensor, k3: torch.Tensor, gray="mean", apply_tanh: bool = True) -> torch.Tensor:
    """frames [F,B,3,H,W] float32 in [-1, 1] or [F,B,H,W,3] uint8 -> cond [F,B,3,H,W] = EdgeExtractor(grey(frame)) in one launch
    (ncahip_clip_cond).  gray: 'mean', 'luma' or three weights; k3: the EdgeExtractor's three 3 x 3 filters."""
    fmt, F_, B, three, H, W = _frames_dims(frames)
    frames = _dev(frames, "frames", frames.dtype)
    assert three == 3, tuple(frames.shape)
    wr, wg, wb = GRAY_WEIGHTS[gray] if isinstance(gray, str) else gray
    k3 = _w(k3.reshape(-1), "k3", frames)
    assert k3.numel() == 27
    cond = torch.empty(F_, B, 3, H, W, device=frames.device, dtype=torch.float32)
    assert cond.numel() * 4 == lib().ncahip_clip_cond_workspace(F_, B, H, W)
    check(lib().ncahip_clip_cond(_p(frames), fmt, _p(k3), wr, wg, wb, int(apply_tanh), _p(cond), F_, B, H, W, _stream()), "clip_cond")
    return cond


OUT_FORMATS = ("rgb24", "i420", "nv12")


class ImageSpec(NamedTuple):
    """The images of a clip call, built and validated by ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W) before
    anything runs: 'rgb24' is float32 [.., c_out, H, W] or uint8 [.., H, W, c_out]; the planar formats 'i420' / 'nv12' are uint8
    [.., 3H/2, W] and need out_dtype=torch.uint8, c_out == 3 and even H, W (ValueError).  fmt: the image format word of the C entry points
    (_clip_fmt(out_dtype), or NCAHIP_CLIP_YUV420(...)); shape: one sample's image -- a driver's images are [n, B, *shape]."""
    out_dtype: torch.dtype
    out_format: str
    yuv_matrix: str
    yuv_range: str
    c_out: int
    H: int
    W: int
    fmt: int
    shape: tuple
    planar: bool

    @classmethod
    def of(cls, out_dtype, out_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited", c_out: int = 3, H: int = 2, W: int = 2):
        if out_format not in OUT_FORMATS:
            raise ValueError(f"out_format must be one of {OUT_FORMATS}, got {out_format!r}")
        if out_format == "rgb24":
            fmt = _clip_fmt(out_dtype)
            shape = (H, W, c_out) if fmt == _capi.CLIP_U8_NHWC else (c_out, H, W)
        else:
            rgb_yuv_coeffs(yuv_matrix, yuv_range)
            if out_dtype != torch.uint8:
                raise ValueError(f"out_format={out_format!r} needs out_dtype=torch.uint8 (planar YUV images are bytes), got {out_dtype}")
            if c_out != 3:
                raise ValueError(f"out_format={out_format!r} needs an RGB image (c_out == 3), got c_out = {c_out}")
            if H % 2 or W % 2:
                raise ValueError(f"out_format={out_format!r} needs even H and W (4:2:0), got {H} x {W}")
            fmt = _capi.clip_yuv420(_capi.YUV_LAYOUTS[out_format], _capi.YUV_MATRICES[yuv_matrix], _capi.YUV_RANGES[yuv_range])
            shape = (3 * H // 2, W)
        return cls(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W, fmt, shape, out_format != "rgb24")

    @property
    def keywords(self) -> dict:
        """The spec as the keywords of the clip drivers and the emit wrappers."""
        return {"out_dtype": self.out_dtype, "out_format": self.out_format, "yuv_matrix": self.yuv_matrix, "yuv_range": self.yuv_range}

    def images(self, n: int, B: int, device, into: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The images tensor [n, B, *shape] of a clip driver: a new one, or the caller's `into` after checking that it is what a new one
        would be."""
        want = (n, B) + self.shape
        if into is None:
            return torch.empty(want, device=device, dtype=self.out_dtype)
        if into.is_cuda and into.dtype == self.out_dtype and tuple(into.shape) == want and into.is_contiguous():
            return into
        raise ValueError(f"images must be a contiguous {self.out_dtype} device tensor {want}, got {tuple(into.shape)} {into.dtype}")


def _clip_img_fmt(out_dtype, *spec) -> int:
    """The format word of ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W)."""
    return ImageSpec.of(out_dtype, *spec).fmt


def clip_emit(x: torch.Tensor, c_out: int = 3, out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709",
              yuv_range: str = "limited") -> torch.Tensor:
    """State [B,C,H,W] -> (clamp(2 x[:, :c_out], -1, 1) + 1) / 2 as float32 [B,c_out,H,W], or truncated to uint8 [B,H,W,c_out].
    out_format 'i420' / 'nv12' (uint8, c_out == 3, even H and W): that uint8 image as planar YUV 4:2:0 [B,3H/2,W], written straight from
    the state -- bit for bit rgb_to_yuv420 of the uint8 image."""
    x = _dev(x, "x")
    B, C, H, W = x.shape
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W)
    img = spec.images(1, B, x.device)[0]
    check(lib().ncahip_clip_emit(_p(x), _p(img), spec.fmt, B, C, c_out, H, W, _stream()), "clip_emit")
    return img


def _clip_persist(nbytes: int, calls: int, device):
    """(ws, nbytes or 0, epoch) of a clip driver's persistent launches: `calls` consecutive epochs of the workspace of `nbytes` bytes
    (0: the persistent kernel is switched off or does not cover the shape), or no workspace.  Never while the current stream is capturing
    a graph: the epochs are kernel arguments, a replay would repeat them (include/ncahip.h), so the drivers then run the per-step kernels."""
    if nbytes and calls < (1 << 20) - 2 and not torch.cuda.is_current_stream_capturing():
        ws, epoch = _persist_workspace(nbytes, device, count=calls)
        return ws, nbytes, epoch
    return None, 0, 0


def _dynca_clip_buffers(x: torch.Tensor, C: int, calls: int, step_n: int, us, seed: int, two_scale: bool, spec: ImageSpec, images):
    """What the two DyNCA clip drivers set up alike: (states, pc, us, seed, images) -- the ring of two state slots with x in the first (x
    may lack the last of the C channels), the coarse scratch of the fused two-scale step, _u_args for all steps and spec.images."""
    B, cx, H, W = x.shape
    us, seed = _u_args(us, calls * step_n, B, H, W, seed)
    states = torch.empty(2, B, C, H, W, device=x.device, dtype=torch.float32)
    states[0, :, :cx].copy_(x)
    pc = torch.empty(B, 4 * C, H // 2, W // 2, device=x.device, dtype=torch.float32) if two_scale else None
    return states, pc, us, seed, spec.images(calls, B, x.device, images)


def dynca_clip(x: torch.Tensor, cond: torch.Tensor, us: Optional[torch.Tensor], w: DyncaWeights, steps_per_frame: int, step_n: int,
               c_out: int = 3, pad_mode: str = "replicate", update_rate: float = 0.5, seed: int = 0, step0: int = 0,
               two_scale: bool = False, out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited",
               images: Optional[torch.Tensor] = None):
    """The video loop over the F frames of cond [F,B,3,H,W] in one C call (ncahip_dynca_clip_f32): per frame steps_per_frame times
    {step_n DyNCA steps, one image}.  us: None (Philox: seed, step0), or the masks / uniforms of all F * steps_per_frame * step_n steps.
    Returns (images [F * steps_per_frame, B, c_out, H, W] float32 or [.., B, H, W, c_out] uint8, final state [B,C,H,W]).
    out_format 'i420' / 'nv12': images [.., B, 3H/2, W] uint8, planar YUV 4:2:0 (clip_emit).  images: a device tensor of the images'
    shape and dtype to write into instead of a new one (what a caller that stages downloads hands in)."""
    x = _dev(x, "x")
    B, C, H, W = x.shape
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W)
    cond = _dev(cond, "cond")
    F_ = cond.shape[0]
    assert cond.shape == (F_, B, 3, H, W), (tuple(cond.shape), tuple(x.shape))
    assert w.c == C and w.k1 == 4 * C + 3, (w.c, w.k1, C)
    calls = F_ * steps_per_frame
    states, pc, us, seed, images = _dynca_clip_buffers(x, C, calls, step_n, us, seed, two_scale, spec, images)
    ws, nbytes, epoch = _clip_persist(lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, w.fc, 3) if persistent_steps else 0, calls, x.device)
    check(lib().ncahip_dynca_clip_f32(_p(states), _p(cond), _p(images), spec.fmt, F_, steps_per_frame, step_n, _p(us), _p(w.w1),
                                      _p(w.b1), _p(w.w2), _p(w.b2), B, C, c_out, H, W, w.fc, PAD_MODES[pad_mode], int(two_scale), update_rate,
                                      seed, step0, _p(pc), _p(ws), nbytes, epoch, _stream()), "dynca_clip")
    return images, states[0]


def clip_gray(frames: torch.Tensor, gray="mean") -> torch.Tensor:
    """frames [F,B,3,H,W] float32 in [-1, 1] or [F,B,H,W,3] uint8 -> grey [F,B,H,W] float32 in one launch (ncahip_clip_gray): what the
    extra-channel models take as their last state channel.  gray: 'mean', 'luma' or three weights."""
    fmt, F_, B, three, H, W = _frames_dims(frames)
    frames = _dev(frames, "frames", frames.dtype)
    assert three == 3, tuple(frames.shape)
    wr, wg, wb = GRAY_WEIGHTS[gray] if isinstance(gray, str) else gray
    out = torch.empty(F_, B, H, W, device=frames.device, dtype=torch.float32)
    check(lib().ncahip_clip_gray(_p(frames), fmt, wr, wg, wb, _p(out), F_, B, H, W, _stream()), "clip_gray")
    return out


def clip_emit_inject(state: torch.Tensor, c_out: int = 3, gray_plane: Optional[torch.Tensor] = None, out_dtype=torch.float32,
                     emit: bool = True, out_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited") -> Optional[torch.Tensor]:
    """One launch (ncahip_clip_emit_inject): the image of state[:, :c_out] as clip_emit (emit=True; returned; out_format as there) and
    gray_plane [B,H,W] written over state[:, C-1] IN PLACE (gray_plane given).  c_out <= C-1.  emit=False: inject only, returns None."""
    if not isinstance(state, torch.Tensor) or not state.is_cuda or state.dtype != torch.float32 or not state.is_contiguous():
        raise _capi.NcaHipError("ncahip: `state` must be a contiguous float32 CUDA (ROCm) tensor -- it is written in place")
    B, C, H, W = state.shape
    if gray_plane is not None:
        gray_plane = _dev(gray_plane, "gray_plane")
        assert gray_plane.numel() == B * H * W, (tuple(gray_plane.shape), tuple(state.shape))
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W)
    img = spec.images(1, B, state.device)[0] if emit else None
    check(lib().ncahip_clip_emit_inject(_p(state), _p(img), spec.fmt, _p(gray_plane), B, C, c_out, H, W, _stream()), "clip_emit_inject")
    return img


def dynca_clip_xc(x: torch.Tensor, gray: torch.Tensor, cond: Optional[torch.Tensor], us: Optional[torch.Tensor], w: DyncaWeights,
                  steps_per_frame: int, step_n: int, c_out: int = 3, pad_mode: str = "replicate", update_rate: float = 0.5, seed: int = 0,
                  step0: int = 0, two_scale: bool = False, out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709",
                  yuv_range: str = "limited", images: Optional[torch.Tensor] = None):
    """dynca_clip for the models whose last state channel is the grey frame (ncahip_dynca_clip_xc_f32): over the F frames of gray
    [F,B,H,W], per frame steps_per_frame times {state[:, -1] = gray[f], step_n DyNCA steps with cond, one image}.  x: the state with all
    C = w.c channels, or with C - 1 (the reference's `h`: the last channel is written before the first call anyway).  cond: ONE map
    [B,2,H,W] (CPE) for all frames, or None.  us, out_format and images as dynca_clip.  Returns (images, final state [B,C,H,W] with the
    evolved last channel)."""
    x = _dev(x, "x")
    B, cx, H, W = x.shape
    C = w.c
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, c_out, H, W)
    gray = _dev(gray, "gray")
    F_ = gray.shape[0]
    assert gray.shape == (F_, B, H, W) and cx in (C - 1, C), (tuple(gray.shape), tuple(x.shape), C)
    c_cond = 0 if cond is None else 2
    if cond is not None:
        cond = _dev(cond, "cond")
        assert cond.shape == (B, 2, H, W), tuple(cond.shape)
    assert w.k1 == 4 * C + c_cond, (w.c, w.k1, c_cond)
    calls = F_ * steps_per_frame
    states, pc, us, seed, images = _dynca_clip_buffers(x, C, calls, step_n, us, seed, two_scale, spec, images)
    ws, nbytes, epoch = _clip_persist(lib().ncahip_dynca_nsteps_persist_workspace(B, C, H, W, w.fc, c_cond) if persistent_steps else 0, calls, x.device)
    check(lib().ncahip_dynca_clip_xc_f32(_p(states), _p(gray), _p(cond), c_cond, _p(images), spec.fmt, F_, steps_per_frame, step_n,
                                         _p(us), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), B, C, c_out, H, W, w.fc, PAD_MODES[pad_mode],
                                         int(two_scale), update_rate, seed, step0, _p(pc), _p(ws), nbytes, epoch, _stream()),
          "dynca_clip_xc")
    return images, states[0]


# ------------------------------------------------------------------------------------ ConditionedNCA
class CondWeights:
    """perception_net.weight [3C,1,3,3]; update_net.out.{0,2,4} weights/biases (nca.py:40-46,99-107)."""

    def __init__(self, wp, w1, b1, w2, b2, w3, like: torch.Tensor):
        self.wp = _w(wp, "wp", like)
        self.w1, self.b1 = _w(w1, "w1", like), _w(b1, "b1", like)
        self.w2, self.b2 = _w(w2, "w2", like), _w(b2, "b2", like)
        self.w3 = _w(w3, "w3", like)
        self.hidden = self.w1.shape[0]
        self.c = self.w3.shape[0]
        assert self.wp.numel() == 27 * self.c and self.w1.numel() == self.hidden * 3 * self.c


def _goal_args(goal, B, C, H, W, dtype=torch.float32):
    if goal is None:
        return None, 0
    goal = _dev(goal, "goal", dtype)
    assert goal.shape[0] == B and goal.shape[2:] == (H, W) and goal.shape[1] <= C
    return goal, goal.shape[1]


def cond_step(x: torch.Tensor, pre_in: Optional[torch.Tensor], goal: Optional[torch.Tensor],
              u: Optional[torch.Tensor], w: CondWeights, alive_ch: int = 3, thr: float = 0.1,
              fire_rate: float = 0.5, lo: float = -10.0, hi: float = 10.0, seed: int = 0, step: int = 0):
    """One fused step; returns (x_pending, pre) -- resolve with cond_finalize (see include/ncahip.h).
    bfloat16 `x` (and `goal`) select the bf16-storage kernel."""
    dt, sfx = _state_dtype(x)
    x = _dev(x, "x", dt)
    B, C, H, W = x.shape
    goal, gch = _goal_args(goal, B, C, H, W, dt)
    if pre_in is not None:
        pre_in = _dev(pre_in, "pre_in", torch.uint8)
    if u is not None:
        u = _dev(u, "u")
        assert u.numel() == B * H * W
    assert w.c == C
    x_out = torch.empty_like(x)
    pre_out = torch.empty(B, H, W, device=x.device, dtype=torch.uint8)
    fn = getattr(lib(), "ncahip_cond_step_fwd_" + sfx)
    check(fn(_p(x), _p(pre_in), _p(x_out), _p(pre_out), _p(goal), gch, _p(u), _p(w.wp), _p(w.w1), _p(w.b1), _p(w.w2),
             _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, alive_ch, thr, fire_rate, lo, hi, seed, step, _stream()),
          "cond_step_fwd_" + sfx)
    return x_out, pre_out


def cond_finalize(x_pend: torch.Tensor, pre: Optional[torch.Tensor], alive_ch: int = 3, thr: float = 0.1,
                  lo: float = -10.0, hi: float = 10.0) -> torch.Tensor:
    dt, sfx = _state_dtype(x_pend)
    x_pend = _dev(x_pend, "x_pend", dt)
    B, C, H, W = x_pend.shape
    if pre is not None:
        pre = _dev(pre, "pre", torch.uint8)
    out = torch.empty_like(x_pend)
    check(getattr(lib(), "ncahip_cond_finalize_" + sfx)(_p(x_pend), _p(pre), _p(out), B, C, H, W, alive_ch, thr, lo, hi,
                                                        _stream()), "cond_finalize_" + sfx)
    return out


def cond_alive(x: torch.Tensor, alive_ch: int = 3, thr: float = 0.1) -> torch.Tensor:
    x = _dev(x, "x")
    B, C, H, W = x.shape
    out = torch.empty(B, 1, H, W, device=x.device, dtype=torch.uint8)
    check(lib().ncahip_cond_alive_u8(_p(x), _p(out), B, C, H, W, alive_ch, thr, _stream()), "cond_alive")
    return out.bool()


def cond_grow(x: torch.Tensor, T: int, goal: Optional[torch.Tensor], us: Optional[torch.Tensor], w: CondWeights,
              alive_ch: int = 3, thr: float = 0.1, fire_rate: float = 0.5, lo: float = -10.0, hi: float = 10.0,
              seed: int = 0, step0: int = 0, keep_history: bool = False):
    """T fused steps + finalize (nca.py:207-208).  Returns (x_T, states, pre).  bfloat16 `x` / `goal` select the
    bf16-storage kernels (forward only)."""
    dt, sfx = _state_dtype(x)
    x = _dev(x, "x", dt)
    B, C, H, W = x.shape
    if T == 0:
        return x.clone(), None, None
    goal, gch = _goal_args(goal, B, C, H, W, dt)
    us, seed = _u_args(us, T, B, H, W, seed)
    assert w.c == C
    if sfx == "f32" and persistent_cond and not torch.cuda.is_current_stream_capturing():
        # small grids (the reference's training shape): the whole grow in ONE launch, one workgroup per tile
        # (ncahip_cond_grow_fwd_persist_f32; its epoch is a kernel argument, so never inside a captured graph).
        # NCAHIP_ERANGE = shape / mode not covered or not every tile gets a CU -> the per-step kernels below
        nbytes = lib().ncahip_cond_grow_persist_workspace(B, C, H, W, w.hidden, gch)
        if nbytes:
            ws, epoch = _persist_workspace(nbytes, x.device)
            out = torch.empty_like(x)
            if keep_history:
                states = torch.empty(T + 1, B, C, H, W, device=x.device, dtype=dt)
                pre = torch.empty(T + 1, B, H, W, device=x.device, dtype=torch.uint8)
                states[0].copy_(x)
            else:
                states, pre = x, None          # ring 2: only slot 0 (the input) is read
            rc = lib().ncahip_cond_grow_fwd_persist_f32(
                _p(states), _p(pre), T + 1 if keep_history else 2, T, _p(out), _p(goal), gch, _p(us), _p(w.wp), _p(w.w1), _p(w.b1),
                _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, alive_ch, thr, fire_rate, lo, hi, seed, step0, _p(ws), nbytes,
                epoch, _stream())
            if rc == 0:
                return (out, states, pre) if keep_history else (out, None, None)
            if rc != _capi.ERANGE:
                check(rc, "cond_grow_fwd_persist")
    ring = T + 1 if keep_history else 2
    states = torch.empty(ring, B, C, H, W, device=x.device, dtype=dt)
    pre = torch.empty(ring, B, H, W, device=x.device, dtype=torch.uint8)
    states[0].copy_(x)
    out = torch.empty_like(x)
    fn = getattr(lib(), "ncahip_cond_grow_fwd_" + sfx)
    check(fn(_p(states), _p(pre), ring, T, _p(out), _p(goal), gch, _p(us), _p(w.wp), _p(w.w1), _p(w.b1), _p(w.w2),
             _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, alive_ch, thr, fire_rate, lo, hi, seed, step0, _stream()),
          "cond_grow_fwd_" + sfx)
    return out, states, pre


def encoder_clip_ok(encoder) -> bool:
    """True for an ImageEncoder that ncahip_clip_encode covers: the drop-in class itself (not a subclass with its own forward), at most 4
    image channels, an embedding of at most 32 channels, the reference's `embed` (3 x 3 conv with bias, ReLU, 3 x 3 conv without)."""
    from .encoder import ImageEncoder
    if type(encoder) is not ImageEncoder:
        return False
    e0, e2 = encoder.embed[0], encoder.embed[2]
    E, ch = e0.out_channels, encoder.channels
    return (1 <= ch <= 4 and 1 <= E <= 32 and e0.bias is not None and e2.bias is None and tuple(e0.weight.shape) == (E, 3 + ch, 3, 3)
            and tuple(e2.weight.shape) == (E, E, 3, 3) and e0.padding == (1, 1) and e2.padding == (1, 1))


def clip_encode(frames: torch.Tensor, encoder_module, dtype=torch.float32) -> torch.Tensor:
    """frames [F,B,ch,H,W] float32 in [0, 1] or [F,B,H,W,3] uint8 -> goal [F,B,E,H,W] = encoder_module(frame) for every frame in one launch
    (ncahip_clip_encode: fixed filters, 3 x 3 conv + bias + ReLU, 3 x 3 conv, on the exact-f32 MFMA).  Inference only: no gradient.
    encoder_module: an ncahip.encoder.ImageEncoder that encoder_clip_ok accepts (anything else raises: there is no fallback here).
    dtype=torch.bfloat16: the goal of a bf16 state (ncahip_clip_encode_bf16: the same kernel, the store rounds) -- bit for bit
    clip_encode(frames, encoder_module).to(torch.bfloat16), without the fp32 goal."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"ncahip: clip_encode writes a float32 or bfloat16 goal, got {dtype}")
    if not encoder_clip_ok(encoder_module):
        raise _capi.NcaHipError("ncahip: clip_encode covers ncahip.encoder.ImageEncoder with at most 4 image channels and an embedding of at most 32")
    fmt, F_, B, ch, H, W = _frames_dims(frames)
    frames = _dev(frames, "frames", frames.dtype)
    enc = encoder_module
    assert ch == enc.channels, (tuple(frames.shape), enc.channels)
    E = enc.embed[0].out_channels
    k3 = _w(torch.cat((enc.sobel_x.weight, enc.sobel_y.weight, enc.laplacian.weight), dim=0).reshape(-1), "k3", frames)
    k5 = _w(enc.gaussian_blur.weight.reshape(-1), "k5", frames)
    w1, b1, w2 = _w(enc.embed[0].weight, "embed.0.weight", frames), _w(enc.embed[0].bias, "embed.0.bias", frames), _w(enc.embed[2].weight, "embed.2.weight", frames)
    goal = torch.empty(F_, B, E, H, W, device=frames.device, dtype=dtype)
    assert goal.numel() * 4 == lib().ncahip_clip_encode_workspace(F_, B, E, H, W)
    fn = lib().ncahip_clip_encode if dtype == torch.float32 else lib().ncahip_clip_encode_bf16
    check(fn(_p(frames), fmt, _p(k3), _p(k5), _p(w1), _p(b1), _p(w2), _p(goal), F_, B, ch, E, H, W, _stream()), "clip_encode")
    return goal


def clip_emit_unit(state: torch.Tensor, out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709",
                   yuv_range: str = "limited") -> torch.Tensor:
    """State [B,C,H,W] -> clamp(state[:, :3], 0, 1) as float32 [B,3,H,W], or truncated to uint8 [B,H,W,3] (ncahip_clip_emit_unit).
    out_format 'i420' / 'nv12' as clip_emit: the uint8 image as planar YUV 4:2:0 [B,3H/2,W].  A bfloat16 state gives the image of the
    widened state, bit for bit (ncahip_clip_emit_unit_bf16)."""
    dt, sfx = _state_dtype(state)
    x = _dev(state, "state", dt)
    B, C, H, W = x.shape
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, 3, H, W)
    img = spec.images(1, B, x.device)[0]
    fn = lib().ncahip_clip_emit_unit if sfx == "f32" else lib().ncahip_clip_emit_unit_bf16
    check(fn(_p(x), _p(img), spec.fmt, B, C, H, W, _stream()), "clip_emit_unit")
    return img


def cond_finalize_emit(x_pend: torch.Tensor, pre: Optional[torch.Tensor], alive_ch: int = 3, thr: float = 0.1, lo: float = -10.0, hi: float = 10.0,
                       out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited"):
    """cond_finalize and clip_emit_unit of its result in ONE launch, for a bfloat16 pending state (ncahip_cond_finalize_emit_bf16): returns
    (x_out, image), bit for bit those of the two calls."""
    x_pend = _dev(x_pend, "x_pend", torch.bfloat16)
    B, C, H, W = x_pend.shape
    if pre is not None:
        pre = _dev(pre, "pre", torch.uint8)
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, 3, H, W)
    out = torch.empty_like(x_pend)
    img = spec.images(1, B, x_pend.device)[0]
    check(lib().ncahip_cond_finalize_emit_bf16(_p(x_pend), _p(pre), _p(out), _p(img), spec.fmt, B, C, H, W, alive_ch, thr, lo, hi, _stream()),
          "cond_finalize_emit")
    return out, img


def cond_clip(x: torch.Tensor, goal: torch.Tensor, us: Optional[torch.Tensor], w: CondWeights, steps_per_frame: int, step_n: int,
              alive_ch: int = 3, thr: float = 0.1, fire_rate: float = 0.5, lo: float = -10.0, hi: float = 10.0, seed: int = 0, step0: int = 0,
              out_dtype=torch.float32, out_format: str = "rgb24", yuv_matrix: str = "bt709", yuv_range: str = "limited",
              images: Optional[torch.Tensor] = None):
    """The ConditionedNCA clip loop over the F frames of goal [F,B,E,H,W] in one C call (ncahip_cond_clip_f32): per frame steps_per_frame times
    {grow(state, step_n) with goal[f], one image clamp(state[:, :3], 0, 1)}.  us: None (Philox: seed, step0), or the masks / uniforms of all
    F * steps_per_frame * step_n steps.  With persistent_cond the calls go to the one-launch grow where it applies.
    Returns (images [F * steps_per_frame, B, 3, H, W] float32 or [.., B, H, W, 3] uint8, final state [B,C,H,W]).  out_format and images as
    dynca_clip.
    A bfloat16 `x` runs ncahip_cond_clip_bf16 (the bf16-storage steps, the finalize and the image of a call in one launch): it needs a
    bfloat16 goal (clip_encode(dtype=torch.bfloat16)) and ignores persistent_cond -- there is no persistent bf16 grow."""
    dt, sfx = _state_dtype(x)
    x = _dev(x, "x", dt)
    B, C, H, W = x.shape
    spec = ImageSpec.of(out_dtype, out_format, yuv_matrix, yuv_range, 3, H, W)
    goal = _dev(goal, "goal", dt)
    F_, gch = goal.shape[0], goal.shape[2]
    assert goal.shape == (F_, B, gch, H, W) and 0 < gch <= C, (tuple(goal.shape), tuple(x.shape))
    calls = F_ * steps_per_frame
    us, seed = _u_args(us, calls * step_n, B, H, W, seed)
    assert w.c == C
    states = torch.empty(4, B, C, H, W, device=x.device, dtype=dt)
    states[0].copy_(x)
    pre = torch.empty(2, B, H, W, device=x.device, dtype=torch.uint8)
    images = spec.images(calls, B, x.device, images)
    if sfx == "bf16":
        check(lib().ncahip_cond_clip_bf16(_p(states), _p(pre), _p(goal), gch, _p(images), spec.fmt, F_, steps_per_frame, step_n, _p(us),
                                          _p(w.wp), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, alive_ch, thr, fire_rate,
                                          lo, hi, seed, step0, _stream()), "cond_clip (bf16)")
        return images, states[0]
    ws, nbytes, epoch = _clip_persist(lib().ncahip_cond_grow_persist_workspace(B, C, H, W, w.hidden, gch) if persistent_cond else 0, calls, x.device)
    check(lib().ncahip_cond_clip_f32(_p(states), _p(pre), _p(goal), gch, _p(images), spec.fmt, F_, steps_per_frame, step_n, _p(us),
                                     _p(w.wp), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W, w.hidden, alive_ch, thr, fire_rate,
                                     lo, hi, seed, step0, _p(ws), nbytes, epoch, _stream()), "cond_clip")
    return images, states[0]


def cond_grow_backward(states: torch.Tensor, pre: torch.Tensor, goal: Optional[torch.Tensor], us: Optional[torch.Tensor],
                       w: CondWeights, g_final: torch.Tensor, T: int, alive_ch: int = 3, thr: float = 0.1,
                       fire_rate: float = 0.5, lo: float = -10.0, hi: float = 10.0, seed: int = 0, step0: int = 0):
    """Backward of cond_grow (states/pre = the keep_history=True buffers).  Returns a dict of gradients in the
    reference parameter layouts: x0, goal, wp [3C,9], w1 [hid,3C], b1, w2 [hid,hid], b2, w3 [C,hid].  A bfloat16 history
    (and goal) selects ncahip_cond_grow_bwd_bf16; g_final and every returned gradient are float32 either way."""
    dt, sfx = _state_dtype(states)
    states, pre, g_final = _dev(states, "states", dt), _dev(pre, "pre", torch.uint8), _dev(g_final.float(), "g_final")
    assert states.shape[0] == T + 1 and pre.shape[0] == T + 1
    _, B, C, H, W = states.shape
    goal, gch = _goal_args(goal, B, C, H, W, dt)
    us, seed = _u_args(us, T, B, H, W, seed)
    dev, f32 = states.device, torch.float32
    hid = w.hidden
    g = {"x0": torch.empty(B, C, H, W, device=dev, dtype=f32),
         "goal": torch.empty(B, gch, H, W, device=dev, dtype=f32) if gch else None,
         "wp": torch.empty(3 * C, 9, device=dev, dtype=f32), "w1": torch.empty(hid, 3 * C, device=dev, dtype=f32),
         "b1": torch.empty(hid, device=dev, dtype=f32), "w2": torch.empty(hid, hid, device=dev, dtype=f32),
         "b2": torch.empty(hid, device=dev, dtype=f32), "w3": torch.empty(C, hid, device=dev, dtype=f32)}
    nbytes = lib().ncahip_cond_grow_bwd_workspace(B, C, H, W, hid)
    ws = _workspace(nbytes, dev)
    check(getattr(lib(), "ncahip_cond_grow_bwd_" + sfx)(
        _p(states), _p(pre), T, _p(goal), gch, _p(us), _p(w.wp), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), _p(w.w3), B, C, H, W,
        hid, alive_ch, thr, fire_rate, lo, hi, seed, step0, _p(g_final), _p(g["x0"]), _p(g["goal"]), _p(g["wp"]), _p(g["w1"]),
        _p(g["b1"]), _p(g["w2"]), _p(g["b2"]), _p(g["w3"]), _p(ws), nbytes, _stream()), "cond_grow_bwd_" + sfx)
    return g


def gram_rows(a: torch.Tensor, b1: torch.Tensor, b2: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """(sum_cells a_i * b_j  [ma, nb],  sum_cells a_i  [ma]) over all B*H*W cells, for a [B,ma,H,W] and b = [b1 | b2] rows
    [B,nb1,H,W] / [B,nb2,H,W]: the weight and bias gradient of a 1x1 conv layer (ncahip_gram_rows_f32).  `out` (a float32
    device vector of ma*nb + ma elements) is ADDED to instead of a fresh result being returned."""
    a, b1 = _dev(a, "a"), _dev(b1, "b1")
    B, ma, H, W = a.shape
    nb1, nb2 = b1.shape[1], 0
    if b2 is not None:
        b2 = _dev(b2, "b2")
        nb2 = b2.shape[1]
    nb = nb1 + nb2
    acc = out is not None
    if acc:
        assert out.is_cuda and out.dtype == torch.float32 and out.numel() == ma * nb + ma and out.is_contiguous()
    else:
        out = torch.empty(ma * nb + ma, device=a.device, dtype=torch.float32)
    nbytes = lib().ncahip_gram_rows_workspace(ma, nb, B, H * W)
    ws = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
    check(lib().ncahip_gram_rows_f32(_p(a), ma, _p(b1), nb1, _p(b2), nb2, B, H * W, _p(out), int(acc), _p(ws), nbytes,
                                     _stream()), "gram_rows")
    return out[:ma * nb].view(ma, nb), out[ma * nb:]


_DYNCA_BWD = {   # dynca_nsteps_backward's drivers: (precision, two_scale, history storage) -> (entry point, its workspace query)
    ("f32", False, "f32"): ("ncahip_dynca_nsteps_bwd_f32", "ncahip_dynca_nsteps_bwd_workspace"),
    ("f32", True, "f32"): ("ncahip_dynca_nsteps_bwd_ms_f32", "ncahip_dynca_nsteps_bwd_ms_workspace"),
    ("f32", False, "bf16"): ("ncahip_dynca_nsteps_bwd_bf16", "ncahip_dynca_nsteps_bwd_bf16_workspace"),
    ("bf16", False, "f32"): ("ncahip_dynca_nsteps_bwd_bfmma_f32", "ncahip_dynca_nsteps_bwd_bfmma_workspace"),
    ("bf16", True, "f32"): ("ncahip_dynca_nsteps_bwd_ms_bfmma_f32", "ncahip_dynca_nsteps_bwd_ms_bfmma_workspace"),
    ("bf16_wide", False, "f32"): ("ncahip_dynca_nsteps_bwd_bfmma_wide_f32", "ncahip_dynca_nsteps_bwd_bfmma_wide_workspace"),
}
# what the backward's `precision` takes beside "f32" (exact): bf16-MFMA training and its wide range -- the range of each, and its words in a refusal
_DYNCA_BFMMA = {"bf16": (dynca_bf16_ok, "the bf16-MFMA DyNCA backward covers C <= 16 and fc <= 128"),
                "bf16_wide": (dynca_bf16_wide_ok, "the wide bf16-MFMA DyNCA backward covers C <= 32 and fc <= 256")}


def dynca_nsteps_backward(states: torch.Tensor, cond: Optional[torch.Tensor], us: Optional[torch.Tensor], w: DyncaWeights,
                          g_final: torch.Tensor, g_states: Optional[torch.Tensor], T: int, pad_mode: str = "replicate",
                          update_rate: float = 0.5, seed: int = 0, step0: int = 0, two_scale: bool = False, precision: str = "f32"):
    """Backward of dynca_nsteps (states = the keep_history=True buffer [T+1,B,C,H,W]): ONE call into the C driver
    ncahip_dynca_nsteps_bwd_f32, which enqueues the whole T-step loop (perception, fused MLP-backward kernel per 128-wide
    slice of the hidden layer, weight-gradient products with the cell axis as K, stencil adjoint) on the current stream with
    one caller-owned workspace.  g_final must already include any cotangent of x_T itself; g_states (optional, [T+1,...])
    adds dL/dx_t cotangents of the intermediate states t < T (forward_nsteps' return_middle_feature).
    precision="bf16": the bf16-MFMA training mode (ncahip_dynca_nsteps_bwd_bfmma_f32 / _ms_bfmma_f32, contract in include/ncahip.h):
    `states` must be a float32 history recorded under dynca_precision("bf16"), C <= 16 and fc <= 128.  precision="bf16_wide": the wide
    range of that mode (ncahip_dynca_nsteps_bwd_bfmma_wide_f32): single-scale, C <= 32 and fc <= 256, a float32 history recorded under
    dynca_precision("bf16_wide"); inside the narrow range that entry point runs the narrow kernels, bit for bit precision="bf16" (with
    two_scale=True the narrow two-scale driver is called; two_scale=True at a wide-only shape raises ValueError).  The ambient
    dynca_precision plays no part here.
    Returns dict x0, w1 [fc,4C+cc], b1, w2 [C,fc], b2."""
    if precision != "f32" and precision not in _DYNCA_BFMMA:
        raise ValueError(f"dynca backward precision must be 'f32', 'bf16' or 'bf16_wide', got {precision!r}")
    if precision == "bf16_wide" and two_scale:      # the wide entry point is single-scale; a narrow two-scale model has the narrow mode's driver
        if not dynca_bf16_ok(states.shape[2], w.fc):
            raise ValueError("ncahip: the wide range of the bf16-MFMA DyNCA backward is single-scale (two_scale=True needs C <= 16 and fc <= 128)")
        precision = "bf16"
    dt, dsfx = _state_dtype(states)      # bfloat16 history: ncahip_dynca_nsteps_bwd_bf16 (storage format only, fp32 gradients)
    states, g = _dev(states, "states", dt), _dev(g_final.float(), "g_final")
    _, B, C, H, W = states.shape
    assert states.shape[0] == T + 1
    c_cond = 0 if cond is None else cond.shape[1]
    if cond is not None:
        cond = _dev(cond, "cond")
    us, seed = _u_args(us, T, B, H, W, seed)
    if g_states is not None:
        g_states = _dev(g_states.float(), "g_states")
        assert g_states.shape == states.shape
    if dsfx == "bf16" and w.fc > 128:
        raise _capi.NcaHipError("ncahip: the bf16-storage DyNCA steps cover fc <= 128")
    dev, f32 = states.device, torch.float32
    fc, k1 = w.fc, 4 * C + c_cond
    out = {"x0": torch.empty(B, C, H, W, device=dev, dtype=f32), "w1": torch.empty(fc, k1, device=dev, dtype=f32),
           "b1": torch.empty(fc, device=dev, dtype=f32), "w2": torch.empty(C, fc, device=dev, dtype=f32),
           "b2": torch.empty(C, device=dev, dtype=f32)}
    assert not (two_scale and dsfx == "bf16"), "the two-scale step is an fp32 kernel"      # two_scale: backward through ncahip_dynca_nsteps_fwd_ms_f32's steps
    if precision in _DYNCA_BFMMA:
        covers, words = _DYNCA_BFMMA[precision]
        if dsfx == "bf16":
            raise _capi.NcaHipError("ncahip: the bf16-MFMA DyNCA backward takes a float32 history (bf16 state storage is out of its scope)")
        if not covers(C, fc):
            raise _capi.NcaHipError(f"ncahip: {words}, got C={C} fc={fc}")
    fn, wsfn = _DYNCA_BWD[precision, bool(two_scale), dsfx]
    nbytes = getattr(lib(), wsfn)(B, C, H, W, fc, c_cond)
    ws = _workspace(nbytes, dev)
    check(getattr(lib(), fn)(_p(states), T, _p(cond), _p(us), _p(w.w1), _p(w.b1), _p(w.w2), _p(w.b2), B, C, H, W, fc, c_cond, PAD_MODES[pad_mode],
                             update_rate, seed, step0, _p(g), _p(g_states), _p(out["x0"]), _p(out["w1"]), _p(out["b1"]), _p(out["w2"]), _p(out["b2"]), _p(ws),
                             nbytes, _stream()), "dynca_nsteps_bwd" + ("_ms" if two_scale else ""))
    return out


# ---------------------------------------------------------------- relaxed-EMD part of the OT appearance loss (csrc/nca_ot.hip)
def ot_gather(t: torch.Tensor, g: torch.Tensor, idx: Optional[torch.Tensor] = None):
    """Feature vectors of one style layer at the sampled positions (ncahip_ot_gather_f32): t [1,c,h,w] the target's map, g [B,c,h,w]
    the generated images', idx [B,N] int32 positions per sample (None: every position, N = h*w).  Returns X, Y [B,N,c] and the
    norms xn, yn [B,N]."""
    t, g = _dev(t, "t"), _dev(g, "g")
    B, c, h, w = g.shape
    assert t.shape == (1, c, h, w), (t.shape, g.shape)
    if idx is not None:
        idx = _dev(idx, "idx", torch.int32)
        assert idx.dim() == 2 and idx.shape[0] == B
    N = h * w if idx is None else idx.shape[1]
    x, y = (torch.empty(B, N, c, device=g.device, dtype=torch.float32) for _ in range(2))
    xn, yn = (torch.empty(B, N, device=g.device, dtype=torch.float32) for _ in range(2))
    check(lib().ncahip_ot_gather_f32(_p(t), _p(g), _p(idx), _p(x), _p(y), _p(xn), _p(yn), B, c, h * w, N, _stream()), "ot_gather")
    return x, y, xn, yn


def ot_gather_backward(dy: torch.Tensor, idx: Optional[torch.Tensor], h: int, w: int) -> torch.Tensor:
    """Adjoint of ot_gather for g: dy [B,N,c] scattered into dL/dg [B,c,h,w] (zero where nothing was sampled)."""
    dy = _dev(dy, "dy")
    B, N, c = dy.shape
    if idx is not None:
        idx = _dev(idx, "idx", torch.int32)
        assert idx.shape == (B, N)
    dg = (torch.zeros if idx is not None else torch.empty)(B, c, h, w, device=dy.device, dtype=torch.float32)
    check(lib().ncahip_ot_gather_bwd_f32(_p(dy), _p(idx), _p(dg), B, c, h * w, N, _stream()), "ot_gather_bwd")
    return dg


def ot_remd(x: torch.Tensor, y: torch.Tensor, xn: torch.Tensor, yn: torch.Tensor):
    """Relaxed EMD over cosine distances d_ij = 1 - <x_i,y_j> / (|x_i| + 1e-10) / (|y_j| + 1e-10) per sample
    (ncahip_ot_remd_fwd_f32): returns dict remd [B], branch [B] (0 rows / 1 columns / 2 equal), rmin, rarg, cmin, carg [B,N]."""
    x, y, xn, yn = _dev(x, "x"), _dev(y, "y"), _dev(xn, "xn"), _dev(yn, "yn")
    B, N, c = x.shape
    assert y.shape == (B, N, c) and xn.shape == (B, N) and yn.shape == (B, N)
    dev, f32, i32 = x.device, torch.float32, torch.int32
    out = {"remd": torch.empty(B, device=dev, dtype=f32), "branch": torch.empty(B, device=dev, dtype=i32),
           "rmin": torch.empty(B, N, device=dev, dtype=f32), "rarg": torch.empty(B, N, device=dev, dtype=i32),
           "cmin": torch.empty(B, N, device=dev, dtype=f32), "carg": torch.empty(B, N, device=dev, dtype=i32)}
    nbytes = lib().ncahip_ot_workspace(B, N, c)
    ws = _workspace(nbytes, dev)
    check(lib().ncahip_ot_remd_fwd_f32(_p(x), _p(y), _p(xn), _p(yn), _p(out["rmin"]), _p(out["rarg"]), _p(out["cmin"]), _p(out["carg"]),
                                       _p(out["remd"]), _p(out["branch"]), B, N, c, _p(ws), nbytes, _stream()), "ot_remd_fwd")
    return out


def ot_remd_backward(x: torch.Tensor, y: torch.Tensor, xn: torch.Tensor, yn: torch.Tensor, rarg: torch.Tensor, carg: torch.Tensor,
                     branch: torch.Tensor, g_remd: torch.Tensor) -> torch.Tensor:
    """dL/dy [B,N,c] of ot_remd given dL/dremd [B] (ncahip_ot_remd_bwd_f32); x is the constant target and gets no gradient."""
    x, y, xn, yn = _dev(x, "x"), _dev(y, "y"), _dev(xn, "xn"), _dev(yn, "yn")
    rarg, carg, branch = _dev(rarg, "rarg", torch.int32), _dev(carg, "carg", torch.int32), _dev(branch, "branch", torch.int32)
    g_remd = _dev(g_remd, "g_remd")
    B, N, c = x.shape
    assert y.shape == (B, N, c) and g_remd.shape == (B,)
    dy = torch.empty_like(y)
    check(lib().ncahip_ot_remd_bwd_f32(_p(x), _p(y), _p(xn), _p(yn), _p(rarg), _p(carg), _p(branch), _p(g_remd), _p(dy), B, N, c,
                                       _stream()), "ot_remd_bwd")
    return dy


# ---------------------------------------------------------------- moment-matching part of the OT appearance loss (csrc/nca_ot_moment.hip)
def ot_moment(x: torch.Tensor, y: torch.Tensor):
    """mean |mx - my| + mean |Cx - Cy| per sample (unbiased covariances) of x, y [B,N,c] as ot_gather returns them
    (ncahip_ot_moment_fwd_f32): returns dict mom [B], and what the backward reads: my [B,c] the column means of y, sgn [B,c] =
    sign(mx - my), S [B,c,c] int8 = sign(Cx - Cy)."""
    x, y = _dev(x, "x"), _dev(y, "y")
    B, N, c = x.shape
    assert y.shape == (B, N, c)
    dev, f32 = x.device, torch.float32
    out = {"mom": torch.empty(B, device=dev, dtype=f32), "my": torch.empty(B, c, device=dev, dtype=f32),
           "sgn": torch.empty(B, c, device=dev, dtype=f32), "S": torch.empty(B, c, c, device=dev, dtype=torch.int8)}
    nbytes = lib().ncahip_ot_moment_workspace(B, N, c)
    ws = _workspace(nbytes, dev)
    check(lib().ncahip_ot_moment_fwd_f32(_p(x), _p(y), _p(out["mom"]), _p(out["my"]), _p(out["sgn"]), _p(out["S"]), B, N, c, _p(ws), nbytes,
                                         _stream()), "ot_moment_fwd")
    return out


def ot_moment_backward(y: torch.Tensor, my: torch.Tensor, sgn: torch.Tensor, S: torch.Tensor, g_mom: torch.Tensor,
                       dy: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dL/dy [B,N,c] of ot_moment given dL/dmom [B] (ncahip_ot_moment_bwd_f32), ADDED to `dy` in place when one is given (the buffer
    ot_remd_backward has just written) and to zeros otherwise; x is the constant target and gets no gradient."""
    y, my, sgn, S, g_mom = _dev(y, "y"), _dev(my, "my"), _dev(sgn, "sgn"), _dev(S, "S", torch.int8), _dev(g_mom, "g_mom")
    B, N, c = y.shape
    assert my.shape == (B, c) and sgn.shape == (B, c) and S.shape == (B, c, c) and g_mom.shape == (B,)
    if dy is None:
        dy = torch.zeros_like(y)
    else:
        assert dy.shape == y.shape and dy.is_contiguous() and _dev(dy, "dy") is dy
    check(lib().ncahip_ot_moment_bwd_f32(_p(y), _p(my), _p(sgn), _p(S), _p(g_mom), _p(dy), B, N, c, _stream()), "ot_moment_bwd")
    return dy


# ---------------------------------------------------------------- crop + resize of uint8 clip frames (csrc/nca_resize.hip)
RESIZE_MAX_DIM, RESIZE_MAX_KSIZE = 16384, 2048      # what ncahip_clip_resize_u8 takes (include/ncahip.h)
_RESIZE_TABLES = {}          # (in, out, resample) -> (k, bounds), numpy, read-only
_RESIZE_TABLES_DEV = {}      # (in, out, resample, device) -> (k, bounds), device copies


def _resize_filter(resample) -> int:
    if resample not in _capi.RESIZE_FILTERS:
        raise ValueError(f"resample must be 'bicubic' or 'lanczos', got {resample!r}")
    return _capi.RESIZE_FILTERS[resample]


def resize_tables(n_in: int, n_out: int, resample: str = "bicubic"):
    """One axis's tables of Pillow's 8-bit resize (include/ncahip.h), from the library's host builder ncahip_resize_tables -- the only
    implementation of that arithmetic; no GPU involved.  Returns numpy int32 (k [n_out, ksize], bounds [n_out, 2] = (xmin, n)):
    output i = clamp((2^21 + sum_{j < n} px[xmin + j] * k[i, j]) >> 22, 0, 255).  Cached; the arrays are read-only."""
    filt = _resize_filter(resample)
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_tables: lengths must be positive, got in={n_in} out={n_out}")
    key = (n_in, n_out, resample)
    tab = _RESIZE_TABLES.get(key)
    if tab is None:
        ksize = lib().ncahip_resize_ksize(n_in, n_out, filt)
        if ksize < 0:
            check(ksize, "resize_ksize")
        k = np.empty((n_out, ksize), dtype=np.int32)
        bounds = np.empty((n_out, 2), dtype=np.int32)
        check(lib().ncahip_resize_tables(n_in, n_out, filt, k.ctypes.data, bounds.ctypes.data, ksize), "resize_tables")
        k.setflags(write=False)
        bounds.setflags(write=False)
        tab = _RESIZE_TABLES[key] = (k, bounds)
    return tab


def _resize_tables_dev(n_in: int, n_out: int, resample: str, device: torch.device):
    key = (int(n_in), int(n_out), resample, device.type, device.index if device.index is not None else torch.cuda.current_device())
    tab = _RESIZE_TABLES_DEV.get(key)
    if tab is None:
        k, bounds = resize_tables(n_in, n_out, resample)
        tab = _RESIZE_TABLES_DEV[key] = (torch.from_numpy(k.copy()).to(device), torch.from_numpy(bounds.copy()).to(device))
    return tab


def _resize_args(shape, size, crop):
    """(N, H, W, out_h, out_w, (x0, y0, w, h)) of a clip_resize call, validated."""
    if len(shape) != 4 or shape[3] != 3:
        raise ValueError(f"frames must be [N,H,W,3] uint8, got {tuple(shape)}")
    N, H, W = int(shape[0]), int(shape[1]), int(shape[2])
    try:
        out_h, out_w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (out_h, out_w), got {size!r}") from None
    if N < 1 or H < 1 or W < 1 or out_h < 1 or out_w < 1:
        raise ValueError(f"clip_resize: frames {tuple(shape)} and size {(out_h, out_w)} must be positive")
    if crop is None:
        box = (0, 0, W, H)
    else:
        try:
            box = tuple(int(v) for v in crop)
        except (TypeError, ValueError):
            raise ValueError(f"crop must be None or a box (x0, y0, w, h), got {crop!r}") from None
        if len(box) != 4:
            raise ValueError(f"crop must be None or a box (x0, y0, w, h), got {crop!r}")
    x0, y0, cw, ch = box
    if cw < 1 or ch < 1 or x0 < 0 or y0 < 0 or x0 + cw > W or y0 + ch > H:
        raise ValueError(f"crop box (x0, y0, w, h) = {box} lies outside the {H} x {W} frame or is empty")
    return N, H, W, out_h, out_w, box


def _clip_resize_launch(frames: torch.Tensor, box, tx, ty, out: torch.Tensor, ws: torch.Tensor) -> None:
    """ncahip_clip_resize_u8 on tensors as they are: frames [N,H,W,3] and out [N,out_h,out_w,3] uint8 and dense, tx = (kx, bx),
    ty = (ky, by) int32 on the device, ws the workspace."""
    N, H, W, _ = frames.shape
    _, out_h, out_w, _ = out.shape
    x0, y0, cw, ch = box
    check(lib().ncahip_clip_resize_u8(_p(frames), N, H, W, x0, y0, cw, ch, _p(tx[0]), _p(tx[1]), tx[0].shape[1], _p(ty[0]), _p(ty[1]),
                                      ty[0].shape[1], _p(out), out_h, out_w, _p(ws), ws.numel() * ws.element_size(), _stream()), "clip_resize")


def _resize_out(out: Optional[torch.Tensor], want: tuple, device) -> torch.Tensor:
    """The result tensor of a resize wrapper: a new one, or the caller's `out` after checking that it is what a new one would be."""
    if out is None:
        return torch.empty(want, device=device, dtype=torch.uint8)
    if out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == want and out.is_contiguous():
        return out
    raise ValueError(f"out must be a contiguous uint8 device tensor {want}, got {tuple(out.shape)} {out.dtype}")


def clip_resize(frames: torch.Tensor, size, crop=None, resample: str = "bicubic", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames [N,H,W,3] uint8 on the device -> [N,out_h,out_w,3] uint8: crop = None or a box (x0, y0, w, h) in pixels, then Pillow's
    8-bit Image.resize to size = (out_h, out_w) with resample 'bicubic' or 'lanczos', bit for bit (ncahip_clip_resize_u8: two launches
    for all N frames).  The tables come from resize_tables; their device copies are cached per (in, out, resample, device).  out: a
    device tensor of the result's shape to write into."""
    _resize_filter(resample)
    frames = _dev(frames, "frames", torch.uint8)
    N, H, W, out_h, out_w, box = _resize_args(frames.shape, size, crop)
    with torch.cuda.device(frames.device):
        tx = _resize_tables_dev(box[2], out_w, resample, frames.device)
        ty = _resize_tables_dev(box[3], out_h, resample, frames.device)
        out = _resize_out(out, (N, out_h, out_w, 3), frames.device)
        ws = _workspace(lib().ncahip_clip_resize_workspace(N, box[3], out_w), frames.device)
        _clip_resize_launch(frames, box, tx, ty, out, ws)
    return out


def _resize_pass_host(img: np.ndarray, k: np.ndarray, bounds: np.ndarray, axis: int) -> np.ndarray:
    """One pass over `axis` of a uint8 array: out[i] = clamp((2^21 + sum_j img[xmin + j] * k[i, j]) >> 22, 0, 255), int32 arithmetic."""
    img = np.moveaxis(img, axis, -1).astype(np.int32)
    out = np.empty(img.shape[:-1] + (k.shape[0],), dtype=np.uint8)
    for i in range(k.shape[0]):
        x, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = img[..., x:x + n] @ k[i, :n] + np.int32(1 << 21)           # int32: the builder checked the bound
        out[..., i] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, -1, axis)


def clip_resize_host(frames, size, crop=None, resample: str = "bicubic"):
    """clip_resize evaluated with numpy on the same tables (resize_tables): the definition in code, bit for bit Pillow's and the kernel's
    result, and the route for CPU tensors.  frames: a uint8 tensor or numpy array [N,H,W,3]; returns the same kind, on the host."""
    _resize_filter(resample)
    as_tensor = isinstance(frames, torch.Tensor)
    arr = frames.detach().cpu().numpy() if as_tensor else np.asarray(frames)
    if arr.dtype != np.uint8:
        raise TypeError(f"ncahip: `frames` must be uint8, got {arr.dtype}")
    N, H, W, out_h, out_w, (x0, y0, cw, ch) = _resize_args(arr.shape, size, crop)
    arr = arr[:, y0:y0 + ch, x0:x0 + cw]
    arr = _resize_pass_host(arr, *resize_tables(cw, out_w, resample), axis=2)        # horizontal first; uint8 in between
    arr = np.ascontiguousarray(_resize_pass_host(arr, *resize_tables(ch, out_h, resample), axis=1))
    return torch.from_numpy(arr) if as_tensor else arr


# ---------------------------------------------------------------- planar YUV 4:2:0 clip frames (csrc/nca_yuv.hip, the loader of nca_resize.hip)
_YUV_COEFFS = {}             # (matrix, range) -> numpy int32 [6], read-only


def yuv_coeffs(yuv_matrix: str = "bt709", yuv_range: str = "limited") -> np.ndarray:
    """(k_y, k_rv, k_gu, k_gv, k_bu, luma offset) of include/ncahip.h's integer YUV -> RGB evaluation, from the library's host builder
    ncahip_yuv_coeffs -- the only implementation of that arithmetic; no GPU involved.  numpy int32 [6], cached and read-only."""
    if yuv_matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"yuv_matrix must be 'bt601' or 'bt709', got {yuv_matrix!r}")
    if yuv_range not in _capi.YUV_RANGES:
        raise ValueError(f"yuv_range must be 'limited' or 'full', got {yuv_range!r}")
    k = _YUV_COEFFS.get((yuv_matrix, yuv_range))
    if k is None:
        k = np.empty(6, dtype=np.int32)
        check(lib().ncahip_yuv_coeffs(_capi.YUV_MATRICES[yuv_matrix], _capi.YUV_RANGES[yuv_range], k.ctypes.data), "yuv_coeffs")
        k.setflags(write=False)
        _YUV_COEFFS[(yuv_matrix, yuv_range)] = k
    return k


def _yuv_layout(pixel_format) -> int:
    if pixel_format not in _capi.YUV_LAYOUTS:
        raise ValueError(f"pixel_format must be 'i420' or 'nv12' here, got {pixel_format!r}")
    return _capi.YUV_LAYOUTS[pixel_format]


def yuv420_frame_size(shape):
    """(h, w) of planar 4:2:0 frames [N, 3h/2, w]; ValueError for any other shape and for odd h or w."""
    if len(shape) != 3 or shape[1] % 3 != 0 or shape[1] < 3 or shape[2] < 2 or shape[2] % 2 != 0:      # rows % 3 == 0: h = 2 rows / 3 is even
        raise ValueError(f"planar YUV 4:2:0 frames must be [N, 3h/2, w] uint8 with even h and w, got {tuple(shape)}")
    return int(shape[1]) // 3 * 2, int(shape[2])


def _yuv_box(shape, crop):
    """(N, h, w, (x0, y0, cw, ch)) of a conversion call, validated with the resize's rules."""
    h, w = yuv420_frame_size(shape)
    N, _, _, _, _, box = _resize_args((shape[0], h, w, 3), (1, 1), crop)
    return N, h, w, box


def yuv420_to_rgb(frames: torch.Tensor, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited", crop=None) -> torch.Tensor:
    """Planar frames [N, 3h/2, w] uint8 on the device ('i420' or 'nv12') -> RGB [N, ch, cw, 3] uint8 of the crop box (x0, y0, w, h) (None:
    the whole frame): ncahip_clip_yuv420_to_rgb_u8, one launch for all N frames, include/ncahip.h's integer arithmetic with nearest
    chroma.  Any alignment of the tensor."""
    layout, k = _yuv_layout(pixel_format), yuv_coeffs(yuv_matrix, yuv_range)
    frames = _dev(frames, "frames", torch.uint8)
    N, h, w, (x0, y0, cw, ch) = _yuv_box(frames.shape, crop)
    with torch.cuda.device(frames.device):
        out = torch.empty(N, ch, cw, 3, device=frames.device, dtype=torch.uint8)
        check(lib().ncahip_clip_yuv420_to_rgb_u8(_p(frames), layout, N, h, w, x0, y0, cw, ch, k.ctypes.data, _p(out), _stream()), "clip_yuv420_to_rgb")
    return out


def yuv420_to_rgb_host(frames, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited", crop=None):
    """yuv420_to_rgb evaluated with numpy on the library's coefficients (yuv_coeffs): the definition in code, bit for bit the kernels'
    result, and the route for CPU tensors.  frames: a uint8 tensor or numpy array [N, 3h/2, w]; returns the same kind, on the host."""
    layout, k = _yuv_layout(pixel_format), yuv_coeffs(yuv_matrix, yuv_range).astype(np.int32)
    as_tensor = isinstance(frames, torch.Tensor)
    arr = frames.detach().cpu().numpy() if as_tensor else np.asarray(frames)
    if arr.dtype != np.uint8:
        raise TypeError(f"ncahip: `frames` must be uint8, got {arr.dtype}")
    N, h, w, (x0, y0, cw, ch) = _yuv_box(arr.shape, crop)
    arr = arr.reshape(N, -1)
    Y = arr[:, :h * w].reshape(N, h, w)
    if layout == _capi.YUV_LAYOUTS["i420"]:
        U = arr[:, h * w:h * w + h * w // 4].reshape(N, h // 2, w // 2)
        V = arr[:, h * w + h * w // 4:].reshape(N, h // 2, w // 2)
    else:
        UV = arr[:, h * w:].reshape(N, h // 2, w // 2, 2)
        U, V = UV[..., 0], UV[..., 1]
    ys, xs = np.arange(y0, y0 + ch), np.arange(x0, x0 + cw)
    y = Y[:, ys][:, :, xs].astype(np.int32) - k[5]
    u = U[:, ys >> 1][:, :, xs >> 1].astype(np.int32) - 128                      # nearest chroma: sample (x >> 1, y >> 1)
    v = V[:, ys >> 1][:, :, xs >> 1].astype(np.int32) - 128
    half = np.int32(1 << 15)
    rgb = np.stack((k[0] * y + k[1] * v + half, k[0] * y + k[2] * u + k[3] * v + half, k[0] * y + k[4] * u + half), axis=-1)   # int32: < 2^26
    out = np.ascontiguousarray(np.clip(rgb >> 16, 0, 255).astype(np.uint8))
    return torch.from_numpy(out) if as_tensor else out


def clip_resize_yuv420(frames: torch.Tensor, size, crop=None, resample: str = "bicubic", pixel_format: str = "i420", yuv_matrix: str = "bt709",
                       yuv_range: str = "limited") -> torch.Tensor:
    """clip_resize of planar frames [N, 3h/2, w] uint8 on the device: ncahip_clip_resize_yuv420_u8, the same two launches, the
    horizontal pass converting in its loader -- bit for bit clip_resize(yuv420_to_rgb(frames, ..., crop=crop), size, None, resample)
    without the full-size RGB image."""
    _resize_filter(resample)
    layout, k = _yuv_layout(pixel_format), yuv_coeffs(yuv_matrix, yuv_range)
    frames = _dev(frames, "frames", torch.uint8)
    h, w = yuv420_frame_size(frames.shape)
    N, _, _, out_h, out_w, box = _resize_args((frames.shape[0], h, w, 3), size, crop)
    with torch.cuda.device(frames.device):
        tx = _resize_tables_dev(box[2], out_w, resample, frames.device)
        ty = _resize_tables_dev(box[3], out_h, resample, frames.device)
        out = torch.empty(N, out_h, out_w, 3, device=frames.device, dtype=torch.uint8)
        ws = _workspace(lib().ncahip_clip_resize_workspace(N, box[3], out_w), frames.device)
        check(lib().ncahip_clip_resize_yuv420_u8(_p(frames), layout, k.ctypes.data, N, h, w, *box, _p(tx[0]), _p(tx[1]), tx[0].shape[1], _p(ty[0]),
                                                 _p(ty[1]), ty[0].shape[1], _p(out), out_h, out_w, _p(ws), ws.numel() * ws.element_size(), _stream()),
              "clip_resize_yuv420")
    return out


# ---------------------------------------------------------------- planar YUV 4:2:0 images out (csrc/nca_yuv_out.hip, the planar emit of nca_clip.hip)
_RGB_YUV_COEFFS = {}         # (matrix, range) -> numpy int32 [10], read-only


def rgb_yuv_coeffs(yuv_matrix: str = "bt709", yuv_range: str = "limited") -> np.ndarray:
    """The (R, G, B) rows of Y, U and V and the luma offset of include/ncahip.h's integer RGB -> YUV evaluation, from the library's host
    builder ncahip_rgb_yuv_coeffs -- the only implementation of that arithmetic; no GPU involved.  numpy int32 [10], cached and read-only."""
    if yuv_matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"yuv_matrix must be 'bt601' or 'bt709', got {yuv_matrix!r}")
    if yuv_range not in _capi.YUV_RANGES:
        raise ValueError(f"yuv_range must be 'limited' or 'full', got {yuv_range!r}")
    k = _RGB_YUV_COEFFS.get((yuv_matrix, yuv_range))
    if k is None:
        k = np.empty(10, dtype=np.int32)
        check(lib().ncahip_rgb_yuv_coeffs(_capi.YUV_MATRICES[yuv_matrix], _capi.YUV_RANGES[yuv_range], k.ctypes.data), "rgb_yuv_coeffs")
        k.setflags(write=False)
        _RGB_YUV_COEFFS[(yuv_matrix, yuv_range)] = k
    return k


def _rgb_images_shape(shape):
    """(N, h, w) of RGB24 images [N,h,w,3] with even h and w; ValueError for anything else."""
    if len(shape) != 4 or shape[3] != 3 or shape[1] < 2 or shape[2] < 2 or shape[1] % 2 or shape[2] % 2:
        raise ValueError(f"RGB images for planar YUV 4:2:0 must be [N,h,w,3] uint8 with even h and w, got {tuple(shape)}")
    return int(shape[0]), int(shape[1]), int(shape[2])


def rgb_to_yuv420(frames: torch.Tensor, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited") -> torch.Tensor:
    """RGB24 images [N,h,w,3] uint8 on the device -> planar YUV 4:2:0 [N, 3h/2, w] uint8 ('i420' or 'nv12'): ncahip_clip_rgb_to_yuv420_u8,
    one launch for all N images, include/ncahip.h's integer arithmetic with the chroma of a 2 x 2 block its mean.  Any alignment."""
    layout, k = _yuv_layout(pixel_format), rgb_yuv_coeffs(yuv_matrix, yuv_range)
    frames = _dev(frames, "frames", torch.uint8)
    N, h, w = _rgb_images_shape(frames.shape)
    with torch.cuda.device(frames.device):
        out = torch.empty(N, 3 * h // 2, w, device=frames.device, dtype=torch.uint8)
        if N:
            check(lib().ncahip_clip_rgb_to_yuv420_u8(_p(frames), layout, N, h, w, k.ctypes.data, _p(out), _stream()), "clip_rgb_to_yuv420")
    return out


def rgb_to_yuv420_host(frames, pixel_format: str, yuv_matrix: str = "bt709", yuv_range: str = "limited"):
    """rgb_to_yuv420 evaluated with numpy on the library's coefficients (rgb_yuv_coeffs): the definition in code, bit for bit the kernels'
    result, and the route for CPU tensors.  frames: a uint8 tensor or numpy array [N,h,w,3]; returns the same kind, on the host."""
    layout, k = _yuv_layout(pixel_format), rgb_yuv_coeffs(yuv_matrix, yuv_range).astype(np.int32)
    as_tensor = isinstance(frames, torch.Tensor)
    arr = frames.detach().cpu().numpy() if as_tensor else np.asarray(frames)
    if arr.dtype != np.uint8:
        raise TypeError(f"ncahip: `frames` must be uint8, got {arr.dtype}")
    N, h, w = _rgb_images_shape(arr.shape)
    rgb = arr.astype(np.int32)
    Y, U, V = rgb_yuv_planes_host(rgb, rgb[:, 0::2, 0::2] + rgb[:, 0::2, 1::2] + rgb[:, 1::2, 0::2] + rgb[:, 1::2, 1::2], k)
    chroma = np.concatenate((U.reshape(N, -1), V.reshape(N, -1)), axis=1) if layout == _capi.YUV_LAYOUTS["i420"] else np.stack((U, V), axis=-1).reshape(N, -1)
    out = np.ascontiguousarray(np.concatenate((Y.reshape(N, -1), chroma), axis=1).reshape(N, 3 * h // 2, w))
    return torch.from_numpy(out) if as_tensor else out


def rgb_yuv_planes_host(rgb: np.ndarray, sums: np.ndarray, k: np.ndarray):
    """The integer contract itself: pixels rgb [..., 3] (0 .. 255) -> Y, and 2 x 2 channel sums [..., 3] (0 .. 1020) -> (U, V); int32 in,
    uint8 out.  k: rgb_yuv_coeffs' ten words."""
    rgb, sums, k = rgb.astype(np.int32), sums.astype(np.int32), k.astype(np.int32)
    Y = k[9] + ((k[0] * rgb[..., 0] + k[1] * rgb[..., 1] + k[2] * rgb[..., 2] + np.int32(1 << 15)) >> 16)
    U = 128 + ((k[3] * sums[..., 0] + k[4] * sums[..., 1] + k[5] * sums[..., 2] + np.int32(1 << 17)) >> 18)          # int32: < 2^27
    V = 128 + ((k[6] * sums[..., 0] + k[7] * sums[..., 1] + k[8] * sums[..., 2] + np.int32(1 << 17)) >> 18)
    return tuple(np.clip(p, 0, 255).astype(np.uint8) for p in (Y, U, V))


def _even_size(size, what: str) -> None:
    """Planar 4:2:0 results have even sides: ValueError for an odd (out_h, out_w)."""
    try:
        odd = any(int(v) % 2 for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"size must be (out_h, out_w), got {size!r}") from None
    if odd:
        raise ValueError(f"{what}: planar YUV 4:2:0 needs an even (out_h, out_w), got {tuple(size)}")


def clip_resize_to_yuv420(frames: torch.Tensor, size, crop=None, resample: str = "bicubic", out_format: str = "i420", yuv_matrix: str = "bt709",
                          yuv_range: str = "limited", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames [N,H,W,3] uint8 on the device -> planar YUV 4:2:0 [N, 3 out_h / 2, out_w] uint8 ('i420' or 'nv12') at size = (out_h, out_w),
    both even: ncahip_clip_resize_u8_yuv420, clip_resize's horizontal pass and a vertical pass that writes the planes -- bit for bit
    rgb_to_yuv420(clip_resize(frames, size, crop, resample), out_format, yuv_matrix, yuv_range) without the full-size RGB image.  out: a
    device tensor of the result's shape to write into."""
    _resize_filter(resample)
    layout, k = _yuv_layout(out_format), rgb_yuv_coeffs(yuv_matrix, yuv_range)
    frames = _dev(frames, "frames", torch.uint8)
    N, H, W, out_h, out_w, box = _resize_args(frames.shape, size, crop)
    _even_size((out_h, out_w), "clip_resize_to_yuv420")
    with torch.cuda.device(frames.device):
        tx = _resize_tables_dev(box[2], out_w, resample, frames.device)
        ty = _resize_tables_dev(box[3], out_h, resample, frames.device)
        out = _resize_out(out, (N, 3 * out_h // 2, out_w), frames.device)
        ws = _workspace(lib().ncahip_clip_resize_workspace(N, box[3], out_w), frames.device)
        check(lib().ncahip_clip_resize_u8_yuv420(_p(frames), N, H, W, *box, _p(tx[0]), _p(tx[1]), tx[0].shape[1], _p(ty[0]), _p(ty[1]),
                                                 ty[0].shape[1], layout, k.ctypes.data, _p(out), out_h, out_w, _p(ws),
                                                 ws.numel() * ws.element_size(), _stream()), "clip_resize_u8_yuv420")
    return out


def clip_resize_to_yuv420_host(frames, size, crop=None, resample: str = "bicubic", out_format: str = "i420", yuv_matrix: str = "bt709",
                               yuv_range: str = "limited"):
    """clip_resize_to_yuv420 on the host: rgb_to_yuv420_host(clip_resize_host(...)) -- the composition is the definition -- and the route
    for CPU tensors.  frames: a uint8 tensor or numpy array [N,H,W,3]; returns the same kind, on the host."""
    _resize_filter(resample)
    _yuv_layout(out_format)
    rgb_yuv_coeffs(yuv_matrix, yuv_range)
    _even_size(_resize_args(tuple(frames.shape), size, crop)[3:5], "clip_resize_to_yuv420")       # before the resize runs
    return rgb_to_yuv420_host(clip_resize_host(frames, size, crop, resample), out_format, yuv_matrix, yuv_range)


# ---------------------------------------------------------------- position sampler of the OT appearance loss (csrc/nca_ot_sample.hip)
_U64_MASK = (1 << 64) - 1
_OT_SAMPLE_DOMAIN = 0x4F5453     # 'OTS': the fourth counter word (include/ncahip.h)


def ot_sample_idx(rows: int, HW: int, n: int, seed: int, row0: int, key_bits: int = 32, device="cuda") -> torch.Tensor:
    """The OT loss's sampled positions, drawn on the device (ncahip_ot_sample_idx): int32 [rows, n]; row r holds, in ascending
    order, the n positions of [0, HW) with the smallest (key, position), the keys being Philox words keyed by `seed` and the
    64-bit row id row0 + r.  Enqueued on the current stream of `device`; nothing synchronises.  key_bits < 32 shortens the keys
    (ties become common: the tie path's test hook)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _capi.NcaHipError("ncahip: ot_sample_idx runs on a CUDA (ROCm) device -- ot_sample_idx_host is the numpy mirror")
    with torch.cuda.device(dev):
        out = torch.empty(max(int(rows), 0), max(int(n), 0), device=dev, dtype=torch.int32)
        check(lib().ncahip_ot_sample_idx(_p(out), int(rows), int(HW), int(n), int(seed) & _U64_MASK, int(row0) & _U64_MASK, int(key_bits),
                                         _stream()), "ot_sample_idx")
    return out


def _philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on numpy uint32 arrays (csrc/nca_common.h nca_philox4x32_10, restated)."""
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for r in range(10):
        p0, p1 = m0 * c0.astype(np.uint64), m1 * c2.astype(np.uint64)           # 32 x 32 -> 64 bits: no overflow
        ka, kb = np.uint32((k0 + r * 0x9E3779B9) & 0xFFFFFFFF), np.uint32((k1 + r * 0xBB67AE85) & 0xFFFFFFFF)
        c0, c1, c2, c3 = (p1 >> s32).astype(np.uint32) ^ c1 ^ ka, p1.astype(np.uint32), (p0 >> s32).astype(np.uint32) ^ c3 ^ kb, p0.astype(np.uint32)
    return c0, c1, c2, c3


def ot_sample_idx_host(rows: int, HW: int, n: int, seed: int, row0: int, key_bits: int = 32, device=None):
    """ot_sample_idx evaluated with numpy: the same definition (include/ncahip.h), bit for bit, as a numpy int32 array [rows, n].
    What the loss uses for CPU features, and what the tests hold the kernel against.  `device` is accepted and ignored."""
    rows, HW, n, key_bits = int(rows), int(HW), int(n), int(key_bits)
    if rows < 1 or n < 1 or n > HW or HW > (1 << 20) or not 1 <= key_bits <= 32:
        raise ValueError(f"ncahip: ot_sample_idx_host: rows={rows} HW={HW} n={n} key_bits={key_bits} outside 1 <= n <= HW <= 2^20, 1 <= key_bits <= 32")
    seed, row0 = int(seed) & _U64_MASK, int(row0) & _U64_MASK
    groups = (HW + 3) // 4
    grp = np.arange(groups, dtype=np.uint32)[None, :]
    pos = np.arange(4 * groups, dtype=np.uint64)[None, :]
    out = np.empty((rows, n), dtype=np.int32)
    step = max(1, (1 << 22) // (4 * groups))                  # rows per block: at most 4 M keys in flight
    for r0 in range(0, rows, step):
        ids = [(row0 + r) & _U64_MASK for r in range(r0, min(rows, r0 + step))]
        lo = np.array([i & 0xFFFFFFFF for i in ids], dtype=np.uint32)[:, None]
        hi = np.array([i >> 32 for i in ids], dtype=np.uint32)[:, None]
        shape = (len(ids), groups)
        w = _philox4x32_10(np.broadcast_to(grp, shape), np.broadcast_to(lo, shape), np.broadcast_to(hi, shape),
                           np.full(shape, _OT_SAMPLE_DOMAIN, dtype=np.uint32), seed & 0xFFFFFFFF, seed >> 32)
        key = np.stack(w, axis=2).reshape(len(ids), 4 * groups) >> np.uint32(32 - key_bits)           # key[r, 4 g + j] = words[j]
        comp = ((key.astype(np.uint64) << np.uint64(20)) | pos)[:, :HW]                              # (key, p) as one integer: p < 2^20
        take = np.partition(comp, n - 1, axis=1)[:, :n] & np.uint64((1 << 20) - 1)
        out[r0:r0 + len(ids)] = np.sort(take, axis=1).astype(np.int32)
    return out


# ---------------------------------------------------------------- sliced-Wasserstein style loss (csrc/nca_slw.hip)
SLW_DIRECTIONS = 32
SLW_MAX_LEN = 65536      # longest row the sort kernels take (include/ncahip.h)
_SLW_MAPS = {}


def slw_nearest_index(m: int, n: int) -> torch.Tensor:
    """The index map j(i) of F.interpolate(mode="nearest") from m to n positions, as a CPU int32 tensor [n]: F.interpolate itself
    applied to arange(m), so that it is the same map by construction (positions below 2^24 are exact in float32)."""
    src = torch.arange(m, dtype=torch.float32).reshape(1, 1, m)
    return torch.nn.functional.interpolate(src, n, mode="nearest").reshape(n).to(torch.int32)


def slw_index_map(m: int, n: int, device) -> torch.Tensor:
    """slw_nearest_index(m, n) on `device`, built once per (m, n, device)."""
    device = torch.device(device)
    key = (m, n, device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else -1))
    jm = _SLW_MAPS.get(key)
    if jm is None:
        jm = _SLW_MAPS[key] = slw_nearest_index(m, n).to(device)
    return jm


def slw_project(source: torch.Tensor, target: torch.Tensor, proj: torch.Tensor):
    """Keys of the sliced-Wasserstein loss (ncahip_slw_project_f32): source [B,c,n], target [1,c,m], proj [c,32] -> ks [B,32,n],
    kt [1,32,m], k[b,p,i] = sum_c x[b,c,i] proj[c,p].  When n == m the two are views of one [(B+1),32,n] buffer, which slw_sort can
    then take in one call."""
    source, target, proj = _dev(source, "source"), _dev(target, "target"), _dev(proj, "proj")
    B, c, n = source.shape
    m = target.shape[2]
    assert target.shape == (1, c, m) and proj.shape == (c, SLW_DIRECTIONS), (source.shape, target.shape, proj.shape)
    if n == m:
        both = torch.empty(B + 1, SLW_DIRECTIONS, n, device=source.device, dtype=torch.float32)
        ks, kt = both[:B], both[B:]
    else:
        ks = torch.empty(B, SLW_DIRECTIONS, n, device=source.device, dtype=torch.float32)
        kt = torch.empty(1, SLW_DIRECTIONS, m, device=source.device, dtype=torch.float32)
    check(lib().ncahip_slw_project_f32(_p(source), _p(target), _p(proj), _p(ks), _p(kt), B, c, n, m, _stream()), "slw_project")
    return ks, kt


def slw_sort(keys: torch.Tensor):
    """Sorts every row of keys [..., n] ascending IN PLACE (ncahip_slw_sort_f32) and returns (keys, perm): perm int32, the original
    position of each sorted element; equal keys keep their original order, as with torch.sort(stable=True)."""
    assert keys.is_contiguous() and _dev(keys, "keys") is keys
    n = keys.shape[-1]
    perm = torch.empty(keys.shape, device=keys.device, dtype=torch.int32)
    check(lib().ncahip_slw_sort_f32(_p(keys), _p(perm), keys.numel() // n, n, _stream()), "slw_sort")
    return keys, perm


def slw_loss(s: torch.Tensor, t: torch.Tensor, jmap: torch.Tensor) -> torch.Tensor:
    """sum (s[b,p,i] - t[p,jmap[i]])^2 over sorted keys s [B,32,n], t [1,32,m] (ncahip_slw_loss_fwd_f32): a 0-dim tensor."""
    s, t, jmap = _dev(s, "s"), _dev(t, "t"), _dev(jmap, "jmap", torch.int32)
    B, _, n = s.shape
    m = t.shape[-1]
    assert s.shape[1] == SLW_DIRECTIONS and t.numel() == SLW_DIRECTIONS * m and jmap.shape == (n,)
    loss = torch.empty(1, device=s.device, dtype=torch.float32)
    nbytes = lib().ncahip_slw_workspace(B, 4, n, m)
    ws = _workspace(nbytes, s.device)
    check(lib().ncahip_slw_loss_fwd_f32(_p(s), _p(t), _p(jmap), _p(loss), B, n, m, _p(ws), nbytes, _stream()), "slw_loss_fwd")
    return loss[0]


def slw_backward(s: torch.Tensor, t: torch.Tensor, jmap: torch.Tensor, perm: torch.Tensor, proj: torch.Tensor,
                 g_loss: torch.Tensor) -> torch.Tensor:
    """dL/dsource [B,c,n] of slw_loss(sort(project(source))) given dL/dloss (one float on the device) (ncahip_slw_bwd_f32): the
    scaled residual scattered through perm, then proj . dk.  The target and proj get no gradient."""
    s, t, jmap, perm = _dev(s, "s"), _dev(t, "t"), _dev(jmap, "jmap", torch.int32), _dev(perm, "perm", torch.int32)
    proj, g_loss = _dev(proj, "proj"), _dev(g_loss, "g_loss")
    B, _, n = s.shape
    m, c = t.shape[-1], proj.shape[0]
    assert perm.shape == s.shape and jmap.shape == (n,) and g_loss.numel() == 1 and proj.shape == (c, SLW_DIRECTIONS)
    ds = torch.empty(B, c, n, device=s.device, dtype=torch.float32)
    nbytes = lib().ncahip_slw_workspace(B, c, n, m)
    ws = _workspace(nbytes, s.device)
    check(lib().ncahip_slw_bwd_f32(_p(s), _p(t), _p(jmap), _p(perm), _p(proj), _p(g_loss), _p(ds), B, c, n, m, _p(ws), nbytes, _stream()),
          "slw_bwd")
    return ds
