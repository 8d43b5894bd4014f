"""Host-side half of the graph-capture contract (no GPU): while the current stream is capturing, ops._clip_persist hands out no
persistent workspace and spends no epoch -- the persistent launches take their epoch as a kernel argument and must stay out of a
captured graph (include/ncahip.h) -- and nothing can opt back in."""
import inspect

import torch


def _patched(monkeypatch, capturing):
    from ncahip import ops
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_PERSIST_WS", {})
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing)
    return ops


def test_clip_persist_hands_out_nothing_while_capturing(monkeypatch):
    ops = _patched(monkeypatch, True)
    dev = torch.device("cpu:0")
    assert ops._clip_persist(512, 6, dev) == (None, 0, 0)
    assert ops._PERSIST_WS == {}                                   # no workspace created, no epoch spent
    ent = [torch.zeros(512, dtype=torch.uint8), 4]
    ops._PERSIST_WS[(0, 0, 512)] = ent
    assert ops._clip_persist(512, 6, dev) == (None, 0, 0)
    assert ops._PERSIST_WS == {(0, 0, 512): ent} and ent[1] == 4   # an existing one is left as it is


def test_clip_persist_outside_a_capture_is_unchanged(monkeypatch):
    """the bookkeeping test_clip_host pins for _persist_workspace(count=k), reached through _clip_persist"""
    ops = _patched(monkeypatch, False)
    dev, LAST = torch.device("cpu:0"), (1 << 20) - 2
    ws, nbytes, e = ops._clip_persist(512, 6, dev)
    assert e == 1 and nbytes == 512 and ws.numel() == 512 and int(ws.sum()) == 0
    ws2, nbytes, e = ops._clip_persist(512, 3, dev)                # epochs 7 .. 9 of the same workspace
    assert ws2 is ws and nbytes == 512 and e == 7 and ops._PERSIST_WS[(0, 0, 512)][1] == 9
    assert ops._clip_persist(0, 6, dev) == (None, 0, 0)            # switched off or a shape that is not covered
    assert ops._clip_persist(512, LAST, dev) == (None, 0, 0)       # more calls than epochs
    assert ops._PERSIST_WS[(0, 0, 512)][1] == 9


def test_nothing_can_ask_for_a_persistent_workspace_while_capturing():
    from ncahip import ops
    assert list(inspect.signature(ops._clip_persist).parameters) == ["nbytes", "calls", "device"]
    for fn in (ops.dynca_clip, ops.dynca_clip_xc, ops.cond_clip):          # the clip drivers' only way to a persistent workspace
        assert "_clip_persist(" in inspect.getsource(fn) and "while_capturing" not in inspect.getsource(fn), fn.__name__
