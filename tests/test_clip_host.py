"""Host-side checks of the clip entry points (no GPU): exports, workspace arithmetic, refusals that come back before any device
call, the Python loop route of stylize_clip on CPU tensors, and the epoch bookkeeping of ops._persist_workspace(count=k).
Every C call here fails its host-side validation: the pointers are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"ncahip_clip_cond_workspace": 4, "ncahip_clip_cond": 13, "ncahip_clip_emit": 9, "ncahip_dynca_clip_f32": 28}
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


def test_clip_symbols_exported_declared_and_bound():
    from ncahip import _capi
    L, protos = lib(), header_prototypes()
    raw = ctypes.CDLL(_capi.LIB_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), f"{name} not exported"
        assert protos.get(name) == nargs, (name, protos.get(name))
        assert len(_capi.SIGNATURES[name]) == nargs
        assert getattr(L, name).argtypes is not None
    assert L.ncahip_clip_cond_workspace.restype is ctypes.c_size_t
    assert (_capi.CLIP_F32_NCHW, _capi.CLIP_U8_NHWC) == (F32, U8)
    hdr = open(os.path.join(ROOT, "include", "ncahip.h")).read()
    assert "#define NCAHIP_CLIP_F32_NCHW 0" in hdr and "#define NCAHIP_CLIP_U8_NHWC  1" in hdr


def test_clip_cond_workspace_arithmetic():
    L = lib()
    assert L.ncahip_clip_cond_workspace(32, 1, 256, 256) == 32 * 3 * 256 * 256 * 4        # 25 MB: the default chunk of stylize_clip
    assert L.ncahip_clip_cond_workspace(3, 2, 5, 7) == 3 * 2 * 3 * 5 * 7 * 4
    assert L.ncahip_clip_cond_workspace(1, 1, 1, 1) == 12
    assert L.ncahip_clip_cond_workspace(2048, 1, 1024, 1024) == 2048 * 3 * 1024 * 1024 * 4    # beyond 2^32 bytes: size_t arithmetic
    for bad in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -1)):
        assert L.ncahip_clip_cond_workspace(*bad) == 0


def test_clip_cond_and_emit_refusals():
    from ncahip import _capi
    L = lib()
    fr, k3, cond = P(0x100000), P(0x200000), P(0x300000)
    ok = dict(frames=fr, fmt=F32, k3=k3, cond=cond, F=2, B=1, H=8, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ncahip_clip_cond(a["frames"], a["fmt"], a["k3"], 1 / 3, 1 / 3, 1 / 3, 1, a["cond"], a["F"], a["B"], a["H"], a["W"], None)

    for kw in (dict(frames=None), dict(k3=None), dict(cond=None)):
        assert call(**kw) == _capi.EINVAL and b"null" in L.ncahip_last_error(), kw
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert call(fmt=-1) == _capi.EINVAL
    for kw in (dict(F=0), dict(F=-3), dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == _capi.EINVAL and b"size" in L.ncahip_last_error(), kw
    assert call(cond=fr) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(cond=P(0x100000 + 2 * 3 * 64 * 4 - 4)) == _capi.EINVAL             # the last float of the frames
    assert call(fmt=U8, cond=P(0x100000 + 2 * 3 * 64 - 1)) == _capi.EINVAL          # the last byte of uint8 frames
    assert call(frames=P(0x100002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()

    st, img = P(0x100000), P(0x200000)
    emit = lambda **kw: (lambda a: L.ncahip_clip_emit(a["st"], a["img"], a["fmt"], a["B"], a["C"], a["c_out"], a["H"], a["W"], None))(
        dict(dict(st=st, img=img, fmt=F32, B=1, C=12, c_out=3, H=8, W=8), **kw))
    assert emit(st=None) == _capi.EINVAL and emit(img=None) == _capi.EINVAL
    assert emit(fmt=7) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert emit(c_out=0) == _capi.EINVAL and emit(c_out=5, C=16) == _capi.EINVAL
    assert emit(c_out=4, C=3) == _capi.EINVAL and b"c_out" in L.ncahip_last_error()
    assert emit(B=0) == _capi.EINVAL and emit(H=0) == _capi.EINVAL
    assert emit(img=st) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()


def test_dynca_clip_refusals_before_any_device_call():
    from ncahip import _capi
    L = lib()
    base = dict(states=P(0x1000000), cond=P(0x2000000), images=P(0x3000000), fmt=F32, F=3, k=2, step_n=4, u=None, w1=P(0x4000000),
                b1=P(0x4100000), w2=P(0x4200000), b2=P(0x4300000), B=1, C=12, c_out=3, H=32, W=48, fc=96, pad=1, two=0, rate=0.5,
                seed=0, step0=0, pc=None, ws=None, ws_bytes=0, epoch0=0)

    def call(**kw):
        a = dict(base, **kw)
        return L.ncahip_dynca_clip_f32(a["states"], a["cond"], a["images"], a["fmt"], a["F"], a["k"], a["step_n"], a["u"], a["w1"], a["b1"],
                                       a["w2"], a["b2"], a["B"], a["C"], a["c_out"], a["H"], a["W"], a["fc"], a["pad"], a["two"], a["rate"],
                                       a["seed"], a["step0"], a["pc"], a["ws"], a["ws_bytes"], a["epoch0"], None)

    for kw in (dict(states=None), dict(cond=None), dict(images=None), dict(w1=None), dict(b2=None)):
        assert call(**kw) == _capi.EINVAL and b"null" in L.ncahip_last_error(), kw
    assert call(two=1, pc=None) == _capi.EINVAL and b"pc_scratch" in L.ncahip_last_error()
    # aliased buffers: the images on the state, the cond on the scratch slot, the images inside cond
    slot = 12 * 32 * 48 * 4
    assert call(images=base["states"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(cond=P(0x1000000 + slot)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(images=P(0x2000000 + 3 * 3 * 32 * 48 * 4 - 4)) == _capi.EINVAL
    assert call(c_out=13) == _capi.EINVAL and call(c_out=4, C=3) == _capi.EINVAL and b"c_out" in L.ncahip_last_error()
    assert call(c_out=5, C=16) == _capi.EINVAL and call(c_out=0) == _capi.EINVAL
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    for kw in (dict(F=0), dict(F=-1), dict(k=0), dict(step_n=0)):
        assert call(**kw) == _capi.EINVAL and b"positive" in L.ncahip_last_error(), kw
    assert call(pad=9) == _capi.EINVAL
    # epochs: calls n = 0 .. F*k - 1 use epoch0 + n, and epoch0 + F*k must stay below 2^20
    ws = P(0x5000000)
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=0) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=(1 << 20) - 6) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=(1 << 20) - 1) == _capi.EINVAL
    need = L.ncahip_dynca_nsteps_persist_workspace(1, 12, 32, 48, 96, 3)
    assert need > 0
    assert call(ws=ws, ws_bytes=need - 1, epoch0=1) == _capi.EINVAL and b"workspace" in L.ncahip_last_error()
    # what the step entry points refuse, the clip refuses with their code
    assert call(C=33) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(fc=2048) == _capi.ERANGE
    assert call(two=1, pc=P(0x6000000), H=31) == _capi.ERANGE and b"even" in L.ncahip_last_error()
    assert call(two=1, pc=P(0x6000000), C=24, c_out=3) == _capi.ERANGE
    assert call(two=1, pc=P(0x6000000), H=2, W=8, pad=3) == _capi.EINVAL and b"coarse grid" in L.ncahip_last_error()
    assert call(u=P(0x7000000), seed=_capi.SEED_U_IS_BITS, rate=1.0) == _capi.ERANGE      # bit-packed masks need 0 <= rate < 1


class _HostModel:
    """The surface stylize_clip's loop route uses, in torch ops on the host (the DyNCA drop-in itself has no CPU path)."""
    device = torch.device("cpu")
    conditioning = "edges"
    perception_scales = [0]
    c_in, c_out = 6, 3

    def __init__(self):
        self.calls = []

    def seed(self, n, size=128):
        sx, sy = (size, size) if isinstance(size, int) else size
        return torch.zeros(n, self.c_in, sy, sx)

    def forward_nsteps(self, h, step_n, cond_img=None):
        assert cond_img.shape == (1, 1) + tuple(h.shape[2:])
        self.calls.append((step_n, cond_img.clone()))
        h = h + 0.05 * step_n * (cond_img + 0.5)
        return h, h[:, :self.c_out] * 2.0


def test_stylize_clip_on_cpu_tensors_takes_the_loop():
    from ncahip import video
    gen = torch.Generator().manual_seed(0)
    frames = torch.rand(3, 3, 5, 7, generator=gen) * 2 - 1
    m = _HostModel()
    images, state = video.stylize_clip(m, frames, step_n=4, steps_per_frame=2)
    assert video.stylize_clip.last_path == "loop"
    assert images.shape == (6, 3, 5, 7) and images.dtype == torch.float32 and state.shape == (1, 6, 5, 7)
    assert float(images.min()) >= 0.0 and float(images.max()) <= 1.0
    assert len(m.calls) == 6 and all(n == 4 for n, _ in m.calls)
    # the default grey is the reference's channel mean; 'luma' is rgb_to_grayscale
    assert torch.equal(m.calls[2][1], frames[1:2].mean(1, keepdim=True))
    m2 = _HostModel()
    video.stylize_clip(m2, frames, step_n=4, steps_per_frame=2, gray="luma")
    assert torch.equal(m2.calls[2][1], video.rgb_to_grayscale(frames[1:2]))
    assert not torch.equal(m.calls[2][1], m2.calls[2][1])
    # uint8 in / uint8 out, channels last; the result does not depend on frames_per_call; a state continues a clip
    u8 = (torch.rand(3, 5, 7, 3, generator=gen) * 256).clamp(0, 255).to(torch.uint8)
    a, sa = video.stylize_clip(_HostModel(), u8, step_n=2, out_dtype=torch.uint8)
    assert a.shape == (3, 5, 7, 3) and a.dtype == torch.uint8 and video.stylize_clip.last_path == "loop"
    b, sb = video.stylize_clip(_HostModel(), u8, step_n=2, out_dtype=torch.uint8, frames_per_call=1)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    c1, s1 = video.stylize_clip(_HostModel(), u8[:2], step_n=2, out_dtype=torch.uint8)
    c2, s2 = video.stylize_clip(_HostModel(), u8[2:], step_n=2, out_dtype=torch.uint8, state=s1)
    assert torch.equal(torch.cat([c1, c2]), a) and torch.equal(s2, sa)
    with pytest.raises(ValueError):
        video.stylize_clip(_HostModel(), frames, gray="green")
    with pytest.raises(ValueError):
        video.stylize_clip(_HostModel(), frames[:, :2])


def test_persist_workspace_reserves_consecutive_epochs(monkeypatch):
    from ncahip import ops
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_PERSIST_WS", {})
    dev, LAST = torch.device("cpu:0"), (1 << 20) - 2        # LAST: the largest epoch a call may use (the kernels take epochs < 2^20)
    ws, e = ops._persist_workspace(512, dev)
    assert e == 1 and ws.numel() == 512 and int(ws.sum()) == 0
    ws2, e = ops._persist_workspace(512, dev, count=6)      # epochs 2 .. 7
    assert e == 2 and ws2 is ws
    assert ops._persist_workspace(512, dev)[1] == 8         # count = 1 stays the default
    assert ops._persist_workspace(512, dev, count=3)[1] == 9
    ent = ops._PERSIST_WS[(0, 0, 512)]
    ws.fill_(7)
    ent[1] = LAST - 6
    ws3, e = ops._persist_workspace(512, dev, count=6)      # exactly fits: epochs LAST - 5 .. LAST
    assert ws3 is ws and e == LAST - 5 and ops._PERSIST_WS[(0, 0, 512)][1] == LAST
    ws4, e = ops._persist_workspace(512, dev)               # none left: a zeroed workspace, restart at 1
    assert e == 1 and int(ws4.sum()) == 0
    ops._PERSIST_WS[(0, 0, 512)][1] = LAST - 5
    ws4.fill_(7)
    ws5, e = ops._persist_workspace(512, dev, count=6)      # five left, six wanted: restart
    assert e == 1 and int(ws5.sum()) == 0 and ops._PERSIST_WS[(0, 0, 512)][1] == 6
    ops._PERSIST_WS[(0, 0, 512)][1] = LAST - 1
    assert ops._persist_workspace(512, dev)[1] == LAST      # the existing one-epoch behaviour at the boundary
    assert ops._persist_workspace(512, dev)[1] == 1
    # the driver accepts exactly what this hands out: epoch0 + count <= 2^20 - 1
    assert LAST - 5 + 6 < (1 << 20)
