"""Order of the host-side refusals of the nine clip entry points that write an image: ncahip_clip_emit, _emit_inject, _emit_unit,
_emit_unit_bf16, ncahip_cond_finalize_emit_bf16 and the drivers ncahip_dynca_clip_f32, ncahip_dynca_clip_xc_f32, ncahip_cond_clip_f32,
ncahip_cond_clip_bf16.  Every call plants two faults (dummy pointers, refused on the host: nothing is dereferenced or launched) and
expects the code and the WHOLE message of the check that comes first, in the style of test_dynca_step_bwd_host.py.  The expected
literals were recorded from the library of the commit before the image record and the single emit launcher went in, before any
source was edited: the table holds the shared bodies to the order every entry point had.  Nothing here needs a GPU."""
import ctypes

import pytest

F32, U8, BAD = 0, 1, 7
I420, NV12 = 0x100 | 0 | 1 << 1, 0x100 | 1 | 1 << 1          # NCAHIP_CLIP_YUV420(layout, BT.709, limited)
BITS = 0x5354494255                                           # NCAHIP_SEED_U_IS_BITS: `u` holds bit-packed fire masks
ST, IMG, GRAY, PRE, WS = 0x1000000, 0x3000000, 0x2000000, 0x1800000, 0x6000000
_W = dict(wp=0x4000000, w1=0x4100000, b1=0x4200000, w2=0x4300000, b2=0x4400000, w3=0x4500000)
_DYNCA = dict(st=ST, cond=GRAY, img=IMG, fmt=F32, F=3, k=2, step_n=4, u=None, B=1, C=12, c_out=3, H=32, W=48, fc=96, pad=1, two=0, rate=0.5,
              seed=0, step0=0, pc=None, ws=None, ws_bytes=1 << 30, epoch0=1, **_W)
_COND = dict(st=ST, pre=PRE, goal=GRAY, gch=16, img=IMG, fmt=F32, F=3, k=2, step_n=4, u=None, B=1, C=20, H=32, W=48, hidden=64, alive=3,
             thr=0.1, rate=0.5, lo=-10.0, hi=10.0, seed=0, step0=0, ws=None, ws_bytes=1 << 30, epoch0=1, **_W)
_EMIT = dict(st=0x100000, img=0x200000, fmt=F32, gray=0x300000, B=1, C=12, c_out=3, H=8, W=8)
_FIN = dict(st=0x100000, pre=0x180000, out=0x200000, img=0x300000, fmt=F32, B=1, C=20, H=8, W=8, alive=3, thr=0.1, lo=-10.0, hi=10.0)
_TAIL = "B C H W hidden alive thr rate lo hi seed step0"
# entry point -> (the arguments of a call that passes every host-side check, their order in the C signature; the stream follows)
CALLS = {
    "ncahip_clip_emit": (_EMIT, "st img fmt B C c_out H W"),
    "ncahip_clip_emit_inject": (dict(_EMIT, C=13), "st img fmt gray B C c_out H W"),
    "ncahip_clip_emit_unit": (dict(_EMIT, C=16), "st img fmt B C H W"),
    "ncahip_clip_emit_unit_bf16": (dict(_EMIT, C=16), "st img fmt B C H W"),
    "ncahip_cond_finalize_emit_bf16": (_FIN, "st pre out img fmt B C H W alive thr lo hi"),
    "ncahip_dynca_clip_f32": (_DYNCA, "st cond img fmt F k step_n u w1 b1 w2 b2 B C c_out H W fc pad two rate seed step0 pc ws ws_bytes epoch0"),
    "ncahip_dynca_clip_xc_f32": (dict(_DYNCA, C=13, gray=PRE, c_cond=2),
                                 "st gray cond c_cond img fmt F k step_n u w1 b1 w2 b2 B C c_out H W fc pad two rate seed step0 pc ws ws_bytes epoch0"),
    "ncahip_cond_clip_f32": (_COND, "st pre goal gch img fmt F k step_n u wp w1 b1 w2 b2 w3 " + _TAIL + " ws ws_bytes epoch0"),
    "ncahip_cond_clip_bf16": (_COND, "st pre goal gch img fmt F k step_n u wp w1 b1 w2 b2 w3 " + _TAIL),
}
_POINTERS = {"st", "img", "gray", "pre", "out", "cond", "goal", "u", "pc", "ws", *_W}


def refusal(entry, **kw):
    """(code, message) of one refused call"""
    from ncahip import _capi
    L = _capi.lib()
    base, order = CALLS[entry]
    a = dict(base, **kw)
    args = [ctypes.c_void_p(a[n]) if n in _POINTERS else a[n] for n in order.split()]
    return getattr(L, entry)(*args, None), L.ncahip_last_error().decode()


BIG = dict(B=256, H=4096, W=4096, u=0x7000000, seed=BITS)     # H*W = 2^24 and B*H*W = 2^32 with bit-packed masks
TWO_FAULTS = [
    # ---- the single-image calls -------------------------------------------------------------------------------------------------
    ('ncahip_clip_emit', 'null+format', dict(st=None, fmt=BAD), (-1, 'clip emit: null pointer')),
    ('ncahip_clip_emit', 'format+size', dict(fmt=BAD, B=0), (-1, 'clip emit: unknown image format 7')),
    ('ncahip_clip_emit', 'size+c_out', dict(H=0, c_out=5), (-1, 'clip emit: bad size')),
    ('ncahip_clip_emit', 'c_out+planar', dict(fmt=I420, c_out=5, H=7), (-1, 'clip emit: c_out=5 must be in 1..4 and at most C=12')),
    ('ncahip_clip_emit', 'planar c_out+odd', dict(fmt=I420, c_out=2, H=7), (-1, 'clip emit: a planar YUV image is made of 3 channels, got c_out=2')),
    ('ncahip_clip_emit', 'odd+misaligned', dict(fmt=NV12, W=7, img=0x200002), (-2, 'clip emit: 4:2:0 images have even sides, got 8 x 7')),
    ('ncahip_clip_emit', 'misaligned+overlap', dict(img=0x100002), (-1, 'clip emit: float32 images must be 4-byte aligned')),
    ('ncahip_clip_emit', 'odd+overlap', dict(fmt=I420, H=7, img=0x100000), (-2, 'clip emit: 4:2:0 images have even sides, got 7 x 8')),
    ('ncahip_clip_emit_inject', 'neither+null', dict(st=None, img=None, gray=None),
     (-1, 'clip emit_inject: neither an image nor a grey plane (null pointer for both halves)')),
    ('ncahip_clip_emit_inject', 'null+format', dict(st=None, fmt=BAD), (-1, 'clip emit: null pointer')),
    ('ncahip_clip_emit_inject', 'format+size', dict(img=None, fmt=BAD, B=0), (-1, 'clip emit: unknown image format 7')),
    ('ncahip_clip_emit_inject', 'planar c_out+odd', dict(fmt=NV12, c_out=4, W=6, H=9),
     (-1, 'clip emit: a planar YUV image is made of 3 channels, got c_out=4')),
    ('ncahip_clip_emit_inject', 'odd+misaligned', dict(fmt=I420, H=9, img=0x200001), (-2, 'clip emit: 4:2:0 images have even sides, got 9 x 8')),
    ('ncahip_clip_emit_inject', 'misaligned+extra', dict(img=0x200002, C=3), (-1, 'clip emit: float32 images must be 4-byte aligned')),
    ('ncahip_clip_emit_inject', 'extra+overlap', dict(C=3, gray=0x100000),
     (-1, 'clip emit_inject: c_out=3 reaches the extra channel (channel C-1 = 2 holds the grey frame: c_out <= C-1)')),
    ('ncahip_clip_emit_unit', 'null+format', dict(img=None, fmt=BAD), (-1, 'clip emit_unit: null pointer')),
    ('ncahip_clip_emit_unit', 'format+size', dict(fmt=0x108, W=0), (-1, 'clip emit_unit: unknown image format 264')),
    ('ncahip_clip_emit_unit', 'size+C2', dict(B=0, C=2), (-1, 'clip emit_unit: bad size')),
    ('ncahip_clip_emit_unit', 'C2+odd', dict(fmt=I420, C=2, H=7), (-1, 'clip emit_unit: the image is state[:, :3], C=2 has fewer than 3 channels')),
    ('ncahip_clip_emit_unit', 'odd+misaligned', dict(fmt=NV12, H=7, img=0x200002), (-2, 'clip emit_unit: 4:2:0 images have even sides, got 7 x 8')),
    ('ncahip_clip_emit_unit', 'misaligned+overlap', dict(img=0x100002), (-1, 'clip emit_unit: float32 images must be 4-byte aligned')),
    ('ncahip_clip_emit_unit_bf16', 'null+format', dict(st=None, fmt=BAD), (-1, 'clip emit_unit: null pointer')),
    ('ncahip_clip_emit_unit_bf16', 'format+size', dict(fmt=2, H=0), (-1, 'clip emit_unit: unknown image format 2')),
    ('ncahip_clip_emit_unit_bf16', 'odd+misaligned', dict(fmt=I420, W=7, img=0x200002), (-2, 'clip emit_unit: 4:2:0 images have even sides, got 8 x 7')),
    ('ncahip_clip_emit_unit_bf16', 'misaligned image+state', dict(img=0x200002, st=0x100001), (-1, 'clip emit_unit: float32 images must be 4-byte aligned')),
    ('ncahip_clip_emit_unit_bf16', 'misaligned state+overlap', dict(st=0x100001, img=0x100004), (-1, 'clip emit_unit: a bf16 state must be 2-byte aligned')),
    ('ncahip_cond_finalize_emit_bf16', 'null+format', dict(pre=None, fmt=BAD), (-1, 'cond_finalize_emit: null pointer')),
    ('ncahip_cond_finalize_emit_bf16', 'format+size', dict(fmt=BAD, B=0), (-1, 'clip emit_unit: unknown image format 7')),
    ('ncahip_cond_finalize_emit_bf16', 'odd+misaligned', dict(fmt=I420, H=7, img=0x300002), (-2, 'clip emit_unit: 4:2:0 images have even sides, got 7 x 8')),
    ('ncahip_cond_finalize_emit_bf16', 'misaligned image+alive', dict(img=0x300002, alive=20), (-1, 'clip emit_unit: float32 images must be 4-byte aligned')),
    ('ncahip_cond_finalize_emit_bf16', 'alive+in-place', dict(alive=20, out=0x100000), (-1, 'cond_finalize_emit: bad size (alive_ch=20 outside C=20)')),
    ('ncahip_cond_finalize_emit_bf16', 'in-place+misaligned', dict(st=0x100001, out=0x100001), (-1, 'cond_finalize_emit: in-place needs alive_ch < 0')),
    ('ncahip_cond_finalize_emit_bf16', 'misaligned state+overlap', dict(st=0x100001, img=0x100004),
     (-1, 'cond_finalize_emit: bf16 states must be 2-byte aligned')),
    # ---- the DyNCA drivers ------------------------------------------------------------------------------------------------------
    ('ncahip_dynca_clip_f32', 'null cond+null', dict(cond=None, st=None), (-1, 'dynca clip: null pointer')),
    ('ncahip_dynca_clip_f32', 'null+format', dict(img=None, fmt=BAD), (-1, 'clip emit: null pointer')),
    ('ncahip_dynca_clip_f32', 'format+size', dict(fmt=BAD, B=0), (-1, 'clip emit: unknown image format 7')),
    ('ncahip_dynca_clip_f32', 'planar c_out+odd', dict(fmt=I420, c_out=2, H=31), (-1, 'clip emit: a planar YUV image is made of 3 channels, got c_out=2')),
    ('ncahip_dynca_clip_f32', 'odd+misaligned', dict(fmt=NV12, W=47, img=IMG + 2), (-2, 'clip emit: 4:2:0 images have even sides, got 32 x 47')),
    ('ncahip_dynca_clip_f32', 'misaligned+count', dict(img=IMG + 2, F=0), (-1, 'clip emit: float32 images must be 4-byte aligned')),
    ('ncahip_dynca_clip_f32', 'count+overlap', dict(step_n=0, img=ST), (-1, 'dynca clip: F, steps_per_frame and step_n must be positive')),
    ('ncahip_dynca_clip_f32', '2^31+overlap', dict(F=1 << 16, k=1 << 15, img=ST), (-1, 'dynca clip: F * steps_per_frame * step_n must stay below 2^31')),
    ('ncahip_dynca_clip_f32', 'overlap+epoch', dict(img=ST, ws=WS, epoch0=0), (-1, 'dynca clip: states, cond and images must not overlap')),
    ('ncahip_dynca_clip_f32', 'epoch+short', dict(ws=WS, epoch0=0, ws_bytes=16),
     (-1, 'dynca clip: epochs epoch0 .. epoch0 + F * steps_per_frame must lie in [1, 2^20) (zero the workspace and restart at 1 when they run out)')),
    ('ncahip_dynca_clip_f32', 'epoch+range', dict(ws=WS, epoch0=(1 << 20) - 6, fc=2000),
     (-1, 'dynca clip: epochs epoch0 .. epoch0 + F * steps_per_frame must lie in [1, 2^20) (zero the workspace and restart at 1 when they run out)')),
    ('ncahip_dynca_clip_f32', 'range+short', dict(ws=WS, ws_bytes=16, fc=2000), (-2, 'dynca step: C=12 fc=2000 c_cond=3 exceeds (32,1024,4)')),
    ('ncahip_dynca_clip_xc_f32', 'null gray+c_cond', dict(gray=None, c_cond=1), (-1, 'dynca clip xc: null pointer')),
    ('ncahip_dynca_clip_xc_f32', 'c_cond+format', dict(c_cond=1, fmt=BAD), (-1, 'dynca clip xc: c_cond=1 must be 0 (no cond map) or 2 (CPE)')),
    ('ncahip_dynca_clip_xc_f32', 'mismatch+null', dict(c_cond=0, st=None), (-1, 'dynca clip xc: cond pointer / c_cond mismatch')),
    ('ncahip_dynca_clip_xc_f32', 'null+format', dict(st=None, fmt=BAD), (-1, 'clip emit: null pointer')),
    ('ncahip_dynca_clip_xc_f32', 'format+size', dict(fmt=BAD, W=0), (-1, 'clip emit: unknown image format 7')),
    ('ncahip_dynca_clip_xc_f32', 'planar c_out+odd', dict(fmt=NV12, c_out=4, H=31), (-1, 'clip emit: a planar YUV image is made of 3 channels, got c_out=4')),
    ('ncahip_dynca_clip_xc_f32', 'odd+extra', dict(fmt=I420, H=31, C=3), (-2, 'clip emit: 4:2:0 images have even sides, got 31 x 48')),
    ('ncahip_dynca_clip_xc_f32', 'extra+count', dict(C=3, F=0),
     (-1, 'dynca clip xc: c_out=3 reaches the extra channel (channel C-1 = 2 holds the grey frame: c_out <= C-1)')),
    ('ncahip_dynca_clip_xc_f32', 'count+overlap', dict(F=-1, gray=ST), (-1, 'dynca clip xc: F, steps_per_frame and step_n must be positive')),
    ('ncahip_dynca_clip_xc_f32', 'overlap+epoch', dict(gray=IMG, ws=WS, epoch0=0), (-1, 'dynca clip xc: states, gray, cond and images must not overlap')),
    ('ncahip_dynca_clip_xc_f32', 'epoch+short', dict(ws=WS, epoch0=1 << 20, ws_bytes=16),
     (-1, 'dynca clip xc: epochs epoch0 .. epoch0 + F * steps_per_frame must lie in [1, 2^20) (zero the workspace and restart at 1 when they run out)')),
    ('ncahip_dynca_clip_xc_f32', 'range+short', dict(ws=WS, ws_bytes=16, fc=2000), (-2, 'dynca step: C=13 fc=2000 c_cond=2 exceeds (32,1024,4)')),
    # ---- the ConditionedNCA drivers ---------------------------------------------------------------------------------------------
    ('ncahip_cond_clip_f32', 'null+format', dict(goal=None, fmt=BAD), (-1, 'cond clip: null pointer')),
    ('ncahip_cond_clip_f32', 'null image+format', dict(img=None, fmt=BAD), (-1, 'clip emit_unit: null pointer')),
    ('ncahip_cond_clip_f32', 'format+size', dict(fmt=BAD, B=0), (-1, 'clip emit_unit: unknown image format 7')),
    ('ncahip_cond_clip_f32', 'odd+misaligned', dict(fmt=I420, H=31, img=IMG + 2), (-2, 'clip emit_unit: 4:2:0 images have even sides, got 31 x 48')),
    ('ncahip_cond_clip_f32', 'misaligned+count', dict(img=IMG + 2, k=0), (-1, 'clip emit_unit: float32 images must be 4-byte aligned')),
    ('ncahip_cond_clip_f32', 'count+range', dict(F=0, hidden=65), (-1, 'cond clip: F, steps_per_frame and step_n must be positive')),
    ('ncahip_cond_clip_f32', '2^31+range', dict(F=1 << 15, k=1 << 15, hidden=65), (-1, 'cond clip: F * steps_per_frame * step_n must stay below 2^31')),
    ('ncahip_cond_clip_f32', 'range+overlap', dict(hidden=65, img=ST), (-2, 'cond step: C=20 hidden=65 exceeds (32,64)')),
    ('ncahip_cond_clip_f32', 'null weight+overlap', dict(w3=None, img=ST), (-1, 'cond step: null pointer')),
    ('ncahip_cond_clip_f32', 'bits+overlap', dict(BIG, img=ST), (-2, 'bit-packed fire masks: B*H*W must stay below 2^32')),
    ('ncahip_cond_clip_f32', 'overlap+epoch', dict(pre=ST, ws=WS, epoch0=0), (-1, 'cond clip: states, pre, goal and images must not overlap')),
    ('ncahip_cond_clip_f32', 'epoch+short', dict(ws=WS, epoch0=0, ws_bytes=16),
     (-1, 'cond clip: epochs epoch0 .. epoch0 + F * steps_per_frame must lie in [1, 2^20) (zero the workspace and restart at 1 when they run out)')),
    ('ncahip_cond_clip_bf16', 'null+format', dict(pre=None, fmt=BAD), (-1, 'cond clip (bf16): null pointer')),
    ('ncahip_cond_clip_bf16', 'format+size', dict(fmt=BAD, H=0), (-1, 'clip emit_unit: unknown image format 7')),
    ('ncahip_cond_clip_bf16', 'odd+misaligned', dict(fmt=NV12, H=31, img=IMG + 2), (-2, 'clip emit_unit: 4:2:0 images have even sides, got 31 x 48')),
    ('ncahip_cond_clip_bf16', 'count+range', dict(step_n=0, C=24), (-1, 'cond clip (bf16): F, steps_per_frame and step_n must be positive')),
    ('ncahip_cond_clip_bf16', 'range+overlap', dict(C=24, img=ST), (-2, 'cond step: C=24 hidden=64 exceeds (20,64)')),
    ('ncahip_cond_clip_bf16', 'range+W10', dict(hidden=65, W=10), (-2, 'cond step: C=20 hidden=65 exceeds (20,64)')),
    ('ncahip_cond_clip_bf16', 'W10+overlap', dict(W=10, img=ST), (-2, 'bf16 cond step: needs W % 4 == 0 and 8-byte aligned state / goal tensors')),
    ('ncahip_cond_clip_bf16', 'misaligned state+overlap', dict(st=ST + 4, goal=ST + 4), (-2, 'bf16 cond step: needs W % 4 == 0 and 8-byte aligned state / goal tensors')),
    ('ncahip_cond_clip_bf16', 'bf16 shape+bits', dict(BIG), (-2, 'bf16 cond step: H*W must be below 2^24')),
    ('ncahip_cond_clip_bf16', 'bits+overlap', dict(BIG, H=2048, B=512, img=ST), (-2, 'bit-packed fire masks: B*H*W must stay below 2^32')),
]


@pytest.mark.parametrize("entry,faults,call,want", TWO_FAULTS, ids=[f"{e[7:]}-{f}" for e, f, _, _ in TWO_FAULTS])
def test_the_first_of_two_faults_is_reported(entry, faults, call, want):
    got = refusal(entry, **call)
    print(f"{entry} [{faults}]: {got}")
    assert got == want, (entry, faults, got, want)
