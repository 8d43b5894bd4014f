"""Host side of the two exact single-step stage entries of the DyNCA backward, ncahip_dynca_step_bwd_f32 and
ncahip_dynca_step_bwd_w2_f32: the order of their refusals.  Every call plants two faults (dummy pointers, refused on the host: nothing is
dereferenced or launched) and expects the code and the whole message of the check that comes first -- the cases, the caller and the
origin of the literals are those of test_dynca_train_bf16_host.py ("precedence: two faults in one call").  Nothing here needs a GPU."""
import pytest

from test_dynca_train_bf16_host import BITS, check_two_faults

TWO_FAULTS = [
    ('ncahip_dynca_step_bwd_f32', 'direction+null', dict(direction=True, g_next=None, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_step_bwd_f32', 'null+C33', dict(g_next=None, C=33, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd: null pointer')),
    ('ncahip_dynca_step_bwd_f32', 'range+alias', dict(g_next=0x3000, fc=129, rate=1.0, seed=BITS),
     (-2, 'dynca step: C=12 fc=129 c_cond=0 exceeds (32,128,4)')),
    ('ncahip_dynca_step_bwd_f32', 'alias+4GiB', dict(g_next=0x3000, H=4096, W=4096, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_f32', 'alias+bits', dict(g_next=0x3000, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_f32', '4GiB+bits', dict(H=4096, W=4096, rate=1.0, seed=BITS),
     (-2, 'dynca step bwd: fc*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
    ('ncahip_dynca_step_bwd_w2_f32', 'direction+null', dict(direction=True, g_next=None),
     (-1, 'dynca step bwd_w2: a direction field is attached (ncahip_dynca_direction) and this entry point does not steer; detach it first')),
    ('ncahip_dynca_step_bwd_w2_f32', 'null+C33', dict(g_next=None, C=33),
     (-1, 'dynca step bwd_w2: null pointer')),
    ('ncahip_dynca_step_bwd_w2_f32', 'range+alias', dict(g_next=0x3000, fc=129),
     (-2, 'dynca step: C=12 fc=129 c_cond=0 exceeds (32,128,4)')),
    ('ncahip_dynca_step_bwd_w2_f32', 'alias+4GiB', dict(g_next=0x3000, H=4096, W=4096),
     (-1, 'dynca step bwd_w2: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_w2_f32', 'alias+short', dict(g_next=0x3000, nbytes=16),
     (-1, 'dynca step bwd_w2: g_next and g_x must not alias')),
    ('ncahip_dynca_step_bwd_w2_f32', 'short+misaligned', dict(nbytes=16, ws=0x10002),
     (-1, 'dynca step bwd_w2: workspace too small')),
    ('ncahip_dynca_step_bwd_w2_f32', 'bits+short', dict(nbytes=16, rate=1.0, seed=BITS),
     (-1, 'dynca step bwd_w2: workspace too small')),
    ('ncahip_dynca_step_bwd_w2_f32', '4GiB+short', dict(nbytes=16, H=4096, W=4096),
     (-2, 'dynca step bwd_w2: fc*H*W*4 must stay below 4 GiB (32-bit store offsets inside a batch item)')),
]


@pytest.mark.parametrize("entry,faults,call,want", TWO_FAULTS, ids=[f"{e[7:]}-{f}" for e, f, _, _ in TWO_FAULTS])
def test_the_first_of_two_faults_is_reported(entry, faults, call, want):
    check_two_faults(entry, faults, call, want)


def test_the_workspace_query_is_host_arithmetic():
    """ncahip_dynca_step_bwd_w2_workspace: 0 for a bad size, positive and monotone in B otherwise"""
    from ncahip import _capi
    q = _capi.lib().ncahip_dynca_step_bwd_w2_workspace
    assert q(0, 12, 16, 16, 96) == 0 and q(1, 12, 16, 16, 0) == 0
    s = [q(B, 12, 64, 64, 96) for B in (1, 2, 4, 8)]
    assert s[0] > 0 and s == sorted(s), s
