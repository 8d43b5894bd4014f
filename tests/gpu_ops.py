"""The one base of the GPU test modules' `ops` fixtures: ncahip.ops in its default state, plus the settings a module asks for."""
import contextlib

import torch


@contextlib.contextmanager
def gpu_ops(persistent_steps=None, persistent_cond=None, force=None, cond_precision=None, dynca_precision=None):
    """with gpu_ops(persistent_steps=False) as ops: ...  -- ncahip.ops after the lane-map selftest, with every process-wide mode at its
    default (ops.reset_modes) and then the given settings applied; whatever the block and its tests left behind is reset on the way out,
    so no module depends on the one that ran before it."""
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    from ncahip import ops
    ops.selftest()
    ops.reset_modes()
    if persistent_steps is not None:
        ops.persistent_steps = persistent_steps
    if persistent_cond is not None:
        ops.persistent_cond = persistent_cond
    if force is not None:
        ops.force_generic(force)
    if cond_precision is not None:
        ops.set_cond_precision(cond_precision)
    if dynca_precision is not None:
        ops.set_dynca_precision(dynca_precision)
    try:
        yield ops
    finally:
        ops.reset_modes()
