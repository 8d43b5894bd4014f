"""Host-side checks of the ConditionedNCA clip entry points (no GPU): exports, workspace arithmetic, every refusal that comes back
before any device call, and the ValueErrors of stylize_clip_conditioned.  Every C call here fails its host-side validation: the
pointers are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"ncahip_clip_encode_workspace": 5, "ncahip_clip_encode": 15, "ncahip_clip_emit_unit": 8, "ncahip_cond_clip_f32": 32}
F32, U8 = 0, 1


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


def test_cond_clip_symbols_exported_declared_and_bound():
    from ncahip import _capi
    L, protos = lib(), header_prototypes()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert len(_capi.SIGNATURES[name]) == nargs
        assert getattr(L, name).argtypes is not None
    assert L.ncahip_clip_encode_workspace.restype is ctypes.c_size_t
    assert L.ncahip_version() == 300


def test_clip_encode_workspace_arithmetic():
    L = lib()
    assert L.ncahip_clip_encode_workspace(8, 1, 16, 256, 256) == 8 * 16 * 256 * 256 * 4       # 34 MB: the default chunk
    assert L.ncahip_clip_encode_workspace(3, 2, 12, 5, 7) == 3 * 2 * 12 * 5 * 7 * 4
    assert L.ncahip_clip_encode_workspace(1, 1, 1, 1, 1) == 4
    assert L.ncahip_clip_encode_workspace(512, 1, 32, 1024, 1024) == 512 * 32 * 1024 * 1024 * 4    # beyond 2^32 bytes: size_t arithmetic
    for bad in ((0, 1, 8, 8, 8), (1, 0, 8, 8, 8), (1, 1, 0, 8, 8), (1, 1, 8, 0, 8), (1, 1, 8, 8, -1), (-2, 1, 8, 8, 8)):
        assert L.ncahip_clip_encode_workspace(*bad) == 0


def test_clip_encode_refusals():
    from ncahip import _capi
    L = lib()
    ok = dict(frames=P(0x100000), fmt=F32, k3=P(0x200000), k5=P(0x210000), w1=P(0x220000), b1=P(0x230000), w2=P(0x240000), goal=P(0x300000),
              F=2, B=1, ch=3, E=16, H=8, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ncahip_clip_encode(a["frames"], a["fmt"], a["k3"], a["k5"], a["w1"], a["b1"], a["w2"], a["goal"], a["F"], a["B"], a["ch"],
                                    a["E"], a["H"], a["W"], None)

    for key in ("frames", "k3", "k5", "w1", "b1", "w2", "goal"):
        assert call(**{key: None}) == _capi.EINVAL and b"null" in L.ncahip_last_error(), key
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert call(fmt=-1) == _capi.EINVAL
    for kw in (dict(F=0), dict(F=-3), dict(B=0), dict(H=0), dict(W=-1), dict(ch=0), dict(E=0)):
        assert call(**kw) == _capi.EINVAL and b"size" in L.ncahip_last_error(), kw
    # aliased in / out: the goal on the frames, on their last element, on a weight
    assert call(goal=ok["frames"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(goal=P(0x100000 + 2 * 3 * 64 * 4 - 4)) == _capi.EINVAL
    assert call(fmt=U8, goal=P(0x100000 + 2 * 3 * 64 - 1)) == _capi.EINVAL
    assert call(goal=ok["w2"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(frames=P(0x100002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()
    # shapes outside the kernel's range
    assert call(E=33) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(ch=5) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(fmt=U8, ch=4) == _capi.ERANGE and b"uint8" in L.ncahip_last_error()
    assert call(fmt=U8, ch=1) == _capi.ERANGE


def test_clip_emit_unit_refusals():
    from ncahip import _capi
    L = lib()
    st, img = P(0x100000), P(0x200000)
    emit = lambda **kw: (lambda a: L.ncahip_clip_emit_unit(a["st"], a["img"], a["fmt"], a["B"], a["C"], a["H"], a["W"], None))(
        dict(dict(st=st, img=img, fmt=F32, B=1, C=20, H=8, W=8), **kw))
    assert emit(st=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert emit(img=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert emit(fmt=7) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert emit(C=2) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error()
    assert emit(B=0) == _capi.EINVAL and emit(H=0) == _capi.EINVAL and b"size" in L.ncahip_last_error()
    assert emit(img=st) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert emit(img=P(0x200001)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()


def test_cond_clip_refusals_before_any_device_call():
    from ncahip import _capi
    L = lib()
    base = dict(states=P(0x1000000), pre=P(0x1800000), goal=P(0x2000000), gch=16, images=P(0x3000000), fmt=F32, F=3, k=2, step_n=4, u=None,
                wp=P(0x4000000), w1=P(0x4100000), b1=P(0x4200000), w2=P(0x4300000), b2=P(0x4400000), w3=P(0x4500000), B=1, C=20, H=32, W=48,
                hidden=64, alive=3, thr=0.1, rate=0.5, lo=-10.0, hi=10.0, seed=0, step0=0, ws=None, ws_bytes=0, epoch0=0)

    def call(**kw):
        a = dict(base, **kw)
        return L.ncahip_cond_clip_f32(a["states"], a["pre"], a["goal"], a["gch"], a["images"], a["fmt"], a["F"], a["k"], a["step_n"], a["u"],
                                      a["wp"], a["w1"], a["b1"], a["w2"], a["b2"], a["w3"], a["B"], a["C"], a["H"], a["W"], a["hidden"],
                                      a["alive"], a["thr"], a["rate"], a["lo"], a["hi"], a["seed"], a["step0"], a["ws"], a["ws_bytes"],
                                      a["epoch0"], None)

    for key in ("states", "pre", "goal", "images", "wp", "w1", "b1", "w2", "b2", "w3"):
        assert call(**{key: None}) == _capi.EINVAL and b"null" in L.ncahip_last_error(), key
    # aliased buffers: the images on the state, the goal on a scratch slot, the pre slots inside the images
    slot = 20 * 32 * 48 * 4
    assert call(images=base["states"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(goal=P(0x1000000 + 3 * slot)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(pre=P(0x3000000 + 6 * 3 * 32 * 48 * 4 - 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    for kw in (dict(F=0), dict(F=-1), dict(k=0), dict(step_n=0), dict(step_n=-2)):
        assert call(**kw) == _capi.EINVAL and b"positive" in L.ncahip_last_error(), kw
    assert call(C=2, gch=2, alive=1) == _capi.EINVAL and b"3 channels" in L.ncahip_last_error()
    assert call(B=0) == _capi.EINVAL and call(W=0) == _capi.EINVAL
    # epochs: calls n = 0 .. F*k - 1 use epoch0 + n, and epoch0 + F*k must stay below 2^20
    ws = P(0x5000000)
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=0) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=(1 << 20) - 6) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=(1 << 20) - 1) == _capi.EINVAL
    need = L.ncahip_cond_grow_persist_workspace(1, 20, 32, 48, 64, 16)
    assert need > 0
    assert call(ws=ws, ws_bytes=need - 1, epoch0=1) == _capi.EINVAL and b"workspace" in L.ncahip_last_error()
    # what the grow drivers refuse, the clip refuses with their code
    assert call(C=33) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(hidden=65) == _capi.ERANGE
    assert call(gch=21) == _capi.EINVAL and b"goal_ch" in L.ncahip_last_error()
    assert call(alive=20) == _capi.EINVAL
    assert call(gch=0) == _capi.EINVAL and b"mismatch" in L.ncahip_last_error()


class _NoGrow(torch.nn.Module):
    """The surface stylize_clip_conditioned validates against; grow must never be reached by a refused call."""
    num_target_channels, num_channels, num_hidden_channels = 3, 20, 16

    def __init__(self, n_target=3):
        super().__init__()
        self.num_target_channels = n_target
        self.p = torch.nn.Parameter(torch.zeros(1))

    def generate_seed(self, n, size=None):
        return torch.zeros(n, self.num_channels, size, size)

    def grow(self, *a):
        raise AssertionError("a refused call reached grow")


def test_stylize_clip_conditioned_value_errors():
    from ncahip import video
    m = _NoGrow()
    f = torch.zeros(2, 3, 8, 8)
    for bad in (f[:, :2], f[0], torch.zeros(2, 8, 8, 3), f.double(), torch.zeros(2, 3, 8, 8, dtype=torch.uint8), f.to(torch.int32)):
        with pytest.raises(ValueError, match="frames must be"):
            video.stylize_clip_conditioned(m, bad)
    with pytest.raises(ValueError, match="num_target_channels"):
        video.stylize_clip_conditioned(_NoGrow(4), f)
    with pytest.raises(ValueError, match="state must be"):
        video.stylize_clip_conditioned(m, f, state=torch.zeros(1, 19, 8, 8))
    with pytest.raises(ValueError, match="state must be"):
        video.stylize_clip_conditioned(m, f, state=torch.zeros(1, 20, 8, 9))
    with pytest.raises(ValueError, match="square"):
        video.stylize_clip_conditioned(m, torch.zeros(2, 3, 8, 12))
    with pytest.raises(ValueError, match="positive"):
        video.stylize_clip_conditioned(m, f, step_n=0)
    with pytest.raises(TypeError):
        video.stylize_clip_conditioned(m, f, out_dtype=torch.float16)
    # uint8 frames are channels last; an empty clip returns no images and the seed
    images, state = video.stylize_clip_conditioned(m, torch.zeros(0, 8, 8, 3, dtype=torch.uint8), out_dtype=torch.uint8)
    assert images.shape == (0, 8, 8, 3) and images.dtype == torch.uint8 and state.shape == (1, 20, 8, 8)
    assert video.stylize_clip_conditioned.last_path == "loop"
