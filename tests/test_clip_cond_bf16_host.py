"""Host-side checks of the ConditionedNCA clip entry points for a bf16 state (no GPU): the four exports, every refusal that comes back
before any device call, and the ValueErrors of stylize_clip_conditioned(precision=...).  Every C call here fails its host-side
validation: the pointers are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"ncahip_clip_encode_bf16": 15, "ncahip_clip_emit_unit_bf16": 8, "ncahip_cond_finalize_emit_bf16": 14, "ncahip_cond_clip_bf16": 29}
F32, U8 = 0, 1
I420, NV12 = 0x100 | 0 | 1 << 1, 0x100 | 1 | 1 << 1          # NCAHIP_CLIP_YUV420(layout, BT.709, limited)


def header_prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ncahip.h")).read(), flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\b(?:int|size_t)\s*(ncahip_\w+)\s*\(([^)]*)\)\s*;", src)}


def P(a):
    return ctypes.c_void_p(a)


def lib():
    from ncahip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_bf16_clip_symbols_exported_declared_and_bound():
    from ncahip import _capi
    L, protos = lib(), header_prototypes()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert len(_capi.SIGNATURES[name]) == nargs
        assert getattr(L, name).argtypes is not None
    # each has the argument list of its fp32 sibling (the driver: without the three persistent-kernel arguments)
    assert _capi.SIGNATURES["ncahip_clip_encode_bf16"] == _capi.SIGNATURES["ncahip_clip_encode"]
    assert _capi.SIGNATURES["ncahip_clip_emit_unit_bf16"] == _capi.SIGNATURES["ncahip_clip_emit_unit"]
    f32 = _capi.SIGNATURES["ncahip_cond_clip_f32"]
    assert _capi.SIGNATURES["ncahip_cond_clip_bf16"] == f32[:-4] + f32[-1:]
    assert L.ncahip_version() == 300


def test_clip_encode_bf16_refusals():
    from ncahip import _capi
    L = lib()
    ok = dict(frames=P(0x100000), fmt=F32, k3=P(0x200000), k5=P(0x210000), w1=P(0x220000), b1=P(0x230000), w2=P(0x240000), goal=P(0x300000),
              F=2, B=1, ch=3, E=16, H=8, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ncahip_clip_encode_bf16(a["frames"], a["fmt"], a["k3"], a["k5"], a["w1"], a["b1"], a["w2"], a["goal"], a["F"], a["B"], a["ch"],
                                         a["E"], a["H"], a["W"], None)

    for key in ("frames", "k3", "k5", "w1", "b1", "w2", "goal"):
        assert call(**{key: None}) == _capi.EINVAL and b"null" in L.ncahip_last_error(), key
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert call(fmt=-1) == _capi.EINVAL
    for kw in (dict(F=0), dict(F=-3), dict(B=0), dict(H=0), dict(W=-1), dict(ch=0), dict(E=0)):
        assert call(**kw) == _capi.EINVAL and b"size" in L.ncahip_last_error(), kw
    # aliased in / out: the goal on the frames, on their last element, on a weight
    assert call(goal=ok["frames"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(goal=P(0x100000 + 2 * 3 * 64 * 4 - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(fmt=U8, goal=P(0x100000 + 2 * 3 * 64 - 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(goal=ok["w2"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    # the goal's bytes are halved: its last bf16 element on the frames' first is refused, the first address past it is not a refusal
    # of the overlap check (frames placed right behind a goal of 2 * 16 * 64 * 2 bytes: the next check that fails is the alignment's)
    gbytes = 2 * 16 * 64 * 2
    assert call(frames=P(0x300000 + gbytes - 2)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(frames=P(0x300000 + gbytes + 2)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    assert call(frames=P(0x100002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    assert call(goal=P(0x300001)) == _capi.EINVAL and b"2-byte aligned" in L.ncahip_last_error()
    # shapes outside the kernel's range
    assert call(E=33) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(ch=5) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(fmt=U8, ch=4) == _capi.ERANGE and b"uint8" in L.ncahip_last_error()
    assert call(fmt=U8, ch=1) == _capi.ERANGE


def test_clip_emit_unit_bf16_refusals():
    from ncahip import _capi
    L = lib()
    st, img = P(0x100000), P(0x200000)
    emit = lambda **kw: (lambda a: L.ncahip_clip_emit_unit_bf16(a["st"], a["img"], a["fmt"], a["B"], a["C"], a["H"], a["W"], None))(
        dict(dict(st=st, img=img, fmt=F32, B=1, C=20, H=8, W=8), **kw))
    assert emit(st=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert emit(img=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert emit(fmt=7) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert emit(fmt=0x108) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert emit(C=2) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error()
    assert emit(B=0) == _capi.EINVAL and emit(H=0) == _capi.EINVAL and b"size" in L.ncahip_last_error()
    assert emit(img=st) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert emit(img=P(0x100000 + 20 * 64 * 2 - 2), fmt=U8) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()      # on the state's last element
    assert emit(img=P(0x200001)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    assert emit(st=P(0x100001)) == _capi.EINVAL and b"2-byte aligned" in L.ncahip_last_error()
    for fmt in (I420, NV12):
        assert emit(fmt=fmt, H=7) == _capi.ERANGE and b"even" in L.ncahip_last_error()
        assert emit(fmt=fmt, W=6, H=9) == _capi.ERANGE and b"even" in L.ncahip_last_error()


def test_cond_finalize_emit_bf16_refusals():
    from ncahip import _capi
    L = lib()
    base = dict(x=P(0x100000), pre=P(0x180000), out=P(0x200000), img=P(0x300000), fmt=F32, B=1, C=20, H=8, W=8, alive=3)

    def call(**kw):
        a = dict(base, **kw)
        return L.ncahip_cond_finalize_emit_bf16(a["x"], a["pre"], a["out"], a["img"], a["fmt"], a["B"], a["C"], a["H"], a["W"], a["alive"], 0.1,
                                                -10.0, 10.0, None)

    for key in ("x", "pre", "out", "img"):
        assert call(**{key: None}) == _capi.EINVAL and b"null" in L.ncahip_last_error(), key
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-1), dict(C=0)):
        assert call(**kw) == _capi.EINVAL and b"size" in L.ncahip_last_error(), kw
    assert call(C=2, alive=1) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error()
    assert call(alive=20) == _capi.EINVAL and b"size" in L.ncahip_last_error()
    assert call(out=base["x"]) == _capi.EINVAL and b"in-place" in L.ncahip_last_error()
    assert call(x=P(0x100001)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    assert call(img=P(0x300002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    # the image on the pending state, on the last element of x_out, on the last byte of pre
    sbytes = 20 * 64 * 2
    assert call(img=base["x"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(img=P(0x200000 + sbytes - 2), fmt=U8) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(img=P(0x180000 + 63), fmt=U8) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    for fmt in (I420, NV12):
        assert call(fmt=fmt, H=7) == _capi.ERANGE and b"even" in L.ncahip_last_error()
    # the shapes of ncahip_cond_finalize_bf16: no W % 4, no C <= 20 -- the only thing left to fail on such a call is a later check
    assert call(W=10, C=24, out=base["x"]) == _capi.EINVAL and b"in-place" in L.ncahip_last_error()


def test_cond_clip_bf16_refusals_before_any_device_call():
    from ncahip import _capi
    L = lib()
    base = dict(states=P(0x1000000), pre=P(0x1800000), goal=P(0x2000000), gch=16, images=P(0x3000000), fmt=F32, F=3, k=2, step_n=4, u=None,
                wp=P(0x4000000), w1=P(0x4100000), b1=P(0x4200000), w2=P(0x4300000), b2=P(0x4400000), w3=P(0x4500000), B=1, C=20, H=32, W=48,
                hidden=64, alive=3, thr=0.1, rate=0.5, lo=-10.0, hi=10.0, seed=0, step0=0)

    def call(**kw):
        a = dict(base, **kw)
        return L.ncahip_cond_clip_bf16(a["states"], a["pre"], a["goal"], a["gch"], a["images"], a["fmt"], a["F"], a["k"], a["step_n"], a["u"],
                                       a["wp"], a["w1"], a["b1"], a["w2"], a["b2"], a["w3"], a["B"], a["C"], a["H"], a["W"], a["hidden"],
                                       a["alive"], a["thr"], a["rate"], a["lo"], a["hi"], a["seed"], a["step0"], None)

    for key in ("states", "pre", "goal", "images", "wp", "w1", "b1", "w2", "b2", "w3"):
        assert call(**{key: None}) == _capi.EINVAL and b"null" in L.ncahip_last_error(), key
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    for kw in (dict(F=0), dict(F=-1), dict(k=0), dict(step_n=0), dict(step_n=-2)):
        assert call(**kw) == _capi.EINVAL and b"positive" in L.ncahip_last_error(), kw
    assert call(C=2, gch=2, alive=1) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error()
    assert call(B=0) == _capi.EINVAL and call(W=0) == _capi.EINVAL
    # what ncahip_cond_grow_fwd_bf16 refuses, with its code
    assert call(C=24) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(C=21, gch=16) == _capi.ERANGE
    assert call(hidden=65) == _capi.ERANGE
    assert call(W=10) == _capi.ERANGE and b"W % 4" in L.ncahip_last_error()
    assert call(states=P(0x1000004)) == _capi.ERANGE and b"8-byte aligned" in L.ncahip_last_error()
    assert call(goal=P(0x2000002)) == _capi.ERANGE and b"8-byte aligned" in L.ncahip_last_error()
    assert call(gch=21) == _capi.EINVAL and b"goal_ch" in L.ncahip_last_error()
    assert call(alive=20) == _capi.EINVAL
    assert call(gch=0) == _capi.EINVAL and b"mismatch" in L.ncahip_last_error()
    for fmt in (I420, NV12):
        assert call(fmt=fmt, H=31) == _capi.ERANGE and b"even" in L.ncahip_last_error()
    # aliased buffers, sizes in bf16 elements: the images on the state, the goal on the last element of scratch slot 3 (and free right
    # behind it: half the fp32 driver's bytes), the pre slots on the last byte of the images
    slot = 20 * 32 * 48 * 2
    assert call(images=base["states"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(goal=P(0x1000000 + 4 * slot - 8)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(pre=P(0x3000000 + 6 * 3 * 32 * 48 * 4 - 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    gbytes = 3 * 16 * 32 * 48 * 2
    assert call(images=P(0x2000000 + gbytes - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()     # on the goal's last elements
    assert call(pre=P(0x1000000 + 4 * slot - 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()


class _NoGrow(torch.nn.Module):
    """The surface stylize_clip_conditioned validates against; grow must never be reached by a refused call."""
    num_target_channels, num_hidden_channels = 3, 16

    def __init__(self, channels=20):
        super().__init__()
        self.num_channels = channels
        self.p = torch.nn.Parameter(torch.zeros(1))

    def generate_seed(self, n, size=None):
        raise AssertionError("a refused call reached generate_seed")

    def grow(self, *a):
        raise AssertionError("a refused call reached grow")


def test_stylize_clip_conditioned_precision_value_errors():
    from ncahip import video
    f = torch.zeros(2, 3, 8, 8)
    for bad in ("fp16", "bf16_wide", "", None):
        with pytest.raises(ValueError, match="precision must be"):
            video.stylize_clip_conditioned(_NoGrow(), f, precision=bad)
    with pytest.raises(ValueError, match="model on the GPU"):
        video.stylize_clip_conditioned(_NoGrow(), f, precision="bf16")                       # a CPU model
    with pytest.raises(ValueError, match="num_channels <= 20"):
        video.stylize_clip_conditioned(_NoGrow(24), f, precision="bf16")
    with pytest.raises(ValueError, match="W % 4 == 0"):
        video.stylize_clip_conditioned(_NoGrow(), torch.zeros(2, 3, 10, 10), precision="bf16")
    with pytest.raises(ValueError, match="W % 4 == 0"):
        video.stylize_clip_conditioned(_NoGrow(), torch.zeros(2, 32, 32, 3, dtype=torch.uint8), precision="bf16", size=(10, 10))
    # the keyword sits where stylize_clip has it, and 'f32' is its default
    import inspect
    names = list(inspect.signature(video.stylize_clip_conditioned).parameters)
    assert names.index("precision") == names.index("resample") + 1
    assert list(inspect.signature(video.stylize_clip).parameters).index("precision") == list(inspect.signature(video.stylize_clip).parameters).index("resample") + 1
    assert inspect.signature(video.stylize_clip_conditioned).parameters["precision"].default == "f32"
