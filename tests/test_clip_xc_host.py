"""Host-side checks of the extra-channel clip entry points (no GPU): ncahip_clip_gray, ncahip_clip_emit_inject and
ncahip_dynca_clip_xc_f32 refuse bad arguments before any device call, each with its code and a word of its message, and
stylize_clip refuses a state with the wrong channel count before it touches the library.
Every C call here fails its host-side validation: the pointers are never dereferenced."""
import ctypes
import os

import pytest
import torch

F32, U8 = 0, 1


def P(a):
    return ctypes.c_void_p(a)


def lib():
    from ncahip import _capi
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_clip_gray_refusals():
    from ncahip import _capi
    L = lib()
    ok = dict(frames=P(0x100000), fmt=F32, gray=P(0x300000), F=2, B=1, H=8, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ncahip_clip_gray(a["frames"], a["fmt"], 1 / 3, 1 / 3, 1 / 3, a["gray"], a["F"], a["B"], a["H"], a["W"], None)

    for kw in (dict(frames=None), dict(gray=None)):
        assert call(**kw) == _capi.EINVAL and b"null" in L.ncahip_last_error(), kw
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert call(fmt=-1) == _capi.EINVAL
    for kw in (dict(F=0), dict(F=-3), dict(B=0), dict(H=0), dict(W=-1)):
        assert call(**kw) == _capi.EINVAL and b"size" in L.ncahip_last_error(), kw
    assert call(gray=ok["frames"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(gray=P(0x100000 + 2 * 3 * 64 * 4 - 4)) == _capi.EINVAL             # the last float of the frames
    assert call(fmt=U8, gray=P(0x100000 + 2 * 3 * 64 - 1)) == _capi.EINVAL          # the last byte of uint8 frames
    assert call(frames=P(0x300000 + 2 * 64 * 4 - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()      # the frames begin on the last float of gray
    assert call(frames=P(0x100002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()


def test_clip_emit_inject_refusals():
    from ncahip import _capi
    L = lib()
    ok = dict(st=P(0x100000), img=P(0x200000), fmt=F32, gray=P(0x300000), B=1, C=13, c_out=3, H=8, W=8)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ncahip_clip_emit_inject(a["st"], a["img"], a["fmt"], a["gray"], a["B"], a["C"], a["c_out"], a["H"], a["W"], None)

    assert call(img=None, gray=None) == _capi.EINVAL and b"neither" in L.ncahip_last_error()      # both halves absent
    assert call(st=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert call(st=None, img=None) == _capi.EINVAL and b"null" in L.ncahip_last_error()
    assert call(fmt=7) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    assert call(c_out=0) == _capi.EINVAL and call(c_out=5, C=16) == _capi.EINVAL and b"c_out" in L.ncahip_last_error()
    # the image never reads the extra channel: c_out == C is refused, in every form of the call
    for kw in (dict(), dict(img=None), dict(gray=None)):
        assert call(c_out=4, C=4, **kw) == _capi.EINVAL and b"extra channel" in L.ncahip_last_error(), kw
        assert call(c_out=3, C=3, **kw) == _capi.EINVAL and b"extra channel" in L.ncahip_last_error(), kw
    assert call(B=0) == _capi.EINVAL and call(H=0) == _capi.EINVAL and b"size" in L.ncahip_last_error()
    slot = 13 * 64 * 4
    assert call(img=ok["st"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(gray=P(0x100000 + slot - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(gray=P(0x200000 + 3 * 64 * 4 - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(fmt=U8, gray=P(0x200000 + 3 * 64 - 1)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(img=P(0x200002)) == _capi.EINVAL and b"aligned" in L.ncahip_last_error()


def _xc_base():
    return dict(states=P(0x1000000), gray=P(0x1800000), cond=P(0x2000000), c_cond=2, images=P(0x3000000), fmt=F32, F=3, k=2, step_n=4, u=None,
                w1=P(0x4000000), b1=P(0x4100000), w2=P(0x4200000), b2=P(0x4300000), B=1, C=13, c_out=3, H=32, W=48, fc=96, pad=1, two=0,
                rate=0.5, seed=0, step0=0, pc=None, ws=None, ws_bytes=0, epoch0=0)


def _xc_call(L, **kw):
    a = dict(_xc_base(), **kw)
    return L.ncahip_dynca_clip_xc_f32(a["states"], a["gray"], a["cond"], a["c_cond"], a["images"], a["fmt"], a["F"], a["k"], a["step_n"], a["u"],
                                      a["w1"], a["b1"], a["w2"], a["b2"], a["B"], a["C"], a["c_out"], a["H"], a["W"], a["fc"], a["pad"], a["two"],
                                      a["rate"], a["seed"], a["step0"], a["pc"], a["ws"], a["ws_bytes"], a["epoch0"], None)


def test_dynca_clip_xc_refusals_before_any_device_call():
    from ncahip import _capi
    L = lib()
    call = lambda **kw: _xc_call(L, **kw)
    for kw in (dict(states=None), dict(gray=None), dict(images=None), dict(w1=None), dict(b2=None)):
        assert call(**kw) == _capi.EINVAL and b"null" in L.ncahip_last_error(), kw
    assert call(fmt=2) == _capi.EINVAL and b"format" in L.ncahip_last_error()
    # c_out: 1..4, and never the extra channel (c_out == C-1 passes that check and stops at the next one, here F = 0)
    assert call(c_out=0) == _capi.EINVAL and call(c_out=5, C=16) == _capi.EINVAL and b"c_out" in L.ncahip_last_error()
    assert call(c_out=4, C=4) == _capi.EINVAL and b"extra channel" in L.ncahip_last_error()
    assert call(c_out=3, C=3) == _capi.EINVAL and b"extra channel" in L.ncahip_last_error()
    assert call(c_out=3, C=4, F=0) == _capi.EINVAL and b"positive" in L.ncahip_last_error()
    assert call(c_out=4, C=5, F=0) == _capi.EINVAL and b"positive" in L.ncahip_last_error()
    # the cond map: CPE (2 channels) or none, and the pointer says the same
    for c_cond in (1, 3, -1):
        assert call(c_cond=c_cond) == _capi.EINVAL and b"c_cond" in L.ncahip_last_error(), c_cond
    assert call(c_cond=0) == _capi.EINVAL and b"mismatch" in L.ncahip_last_error()             # a cond pointer with c_cond = 0
    assert call(cond=None) == _capi.EINVAL and b"mismatch" in L.ncahip_last_error()            # no pointer with c_cond = 2
    # overlaps among states (2 slots), gray [F,B,H,W], cond (ONE map [B,2,H,W]) and images
    slot, plane = 13 * 32 * 48 * 4, 32 * 48 * 4
    b = _xc_base()
    assert call(images=b["states"]) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(cond=P(0x1000000 + slot)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()        # on the scratch slot
    assert call(gray=P(0x1000000 + 2 * slot - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(gray=P(0x2000000 + 2 * plane - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()     # the last float of cond
    assert call(images=P(0x1800000 + 3 * plane - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()   # the last float of gray
    assert call(images=P(0x2000000 + 2 * plane - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    assert call(c_cond=0, cond=None, gray=P(0x1000000 + 2 * slot - 4)) == _capi.EINVAL and b"overlap" in L.ncahip_last_error()
    for kw in (dict(F=0), dict(F=-1), dict(k=0), dict(step_n=0)):
        assert call(**kw) == _capi.EINVAL and b"positive" in L.ncahip_last_error(), kw
    assert call(pad=9) == _capi.EINVAL
    assert call(two=1, pc=None) == _capi.EINVAL and b"pc_scratch" in L.ncahip_last_error()
    # epochs: calls n = 0 .. F*k - 1 use epoch0 + n, and epoch0 + F*k must stay below 2^20
    ws = P(0x5000000)
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=0) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    assert call(ws=ws, ws_bytes=1 << 30, epoch0=(1 << 20) - 6) == _capi.EINVAL and b"epoch" in L.ncahip_last_error()
    need = L.ncahip_dynca_nsteps_persist_workspace(1, 13, 32, 48, 96, 2)
    assert need > 0
    assert call(ws=ws, ws_bytes=need - 1, epoch0=1) == _capi.EINVAL and b"workspace" in L.ncahip_last_error()
    # what the step entry points refuse, the clip refuses with their code
    assert call(C=33) == _capi.ERANGE and b"exceeds" in L.ncahip_last_error()
    assert call(fc=2048) == _capi.ERANGE
    assert call(two=1, pc=P(0x6000000), H=31) == _capi.ERANGE and b"even" in L.ncahip_last_error()
    assert call(u=P(0x7000000), seed=_capi.SEED_U_IS_BITS, rate=1.0) == _capi.ERANGE      # bit-packed masks need 0 <= rate < 1


def test_the_edge_driver_keeps_its_codes_and_messages():
    """ncahip_dynca_clip_f32 shares its body with the new export: c_out == C stays legal there, and its messages keep their prefix."""
    from ncahip import _capi
    L = lib()
    a = _xc_base()

    def call(**kw):
        b = dict(a, **kw)
        return L.ncahip_dynca_clip_f32(b["states"], b["cond"], b["images"], b["fmt"], b["F"], b["k"], b["step_n"], b["u"], b["w1"], b["b1"],
                                       b["w2"], b["b2"], b["B"], b["C"], b["c_out"], b["H"], b["W"], b["fc"], b["pad"], b["two"], b["rate"],
                                       b["seed"], b["step0"], b["pc"], b["ws"], b["ws_bytes"], b["epoch0"], None)

    assert call(c_out=4, C=4, F=0) == _capi.EINVAL and L.ncahip_last_error().startswith(b"dynca clip: F")      # past the c_out check
    assert call(images=a["states"]) == _capi.EINVAL and b"dynca clip: states, cond and images must not overlap" in L.ncahip_last_error()
    assert call(cond=None) == _capi.EINVAL and b"dynca clip: null" in L.ncahip_last_error()


class _Poisoned:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the state was checked")


def test_stylize_clip_refuses_a_c_in_channel_state_before_the_library(monkeypatch):
    from ncahip import _capi, ops, video
    from ncahip.models import dynca_extra
    m = dynca_extra.DyNCA(13, 3, fc_dim=96, padding_mode="circular", pos_emb="CPE", device=torch.device("cpu"))
    frames = torch.zeros(2, 3, 8, 12)
    monkeypatch.setattr(_capi, "lib", lambda: _Poisoned())
    monkeypatch.setattr(ops, "lib", lambda: _Poisoned())
    for bad in (torch.zeros(1, 13, 8, 12), torch.zeros(1, 11, 8, 12), torch.zeros(12, 8, 12)):
        with pytest.raises(ValueError, match="c_in - 1"):
            video.stylize_clip(m, frames, state=bad)
    assert m.seed(1, size=(12, 8)).shape == (1, 12, 8, 12)              # what the model itself seeds: the accepted channel count
