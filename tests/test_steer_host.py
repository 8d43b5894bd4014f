"""Host side of steered DyNCA perception (ncahip.steer, ncahip_dynca_direction in include/ncahip.h): the direction fields against an
independent float64 evaluation of docs/dynca.js:209-225, the weight fold for a uniform angle, the positional-encoding rotation, the
C entry point's argument and attachment checks (no device: every call below is refused on the host before any launch), and the
models' refusal of a steered step under autograd.  The kernels themselves: test_gpu_steer.py."""
import ctypes
import math

import pytest
import torch

SIZES = [(8, 8), (7, 9), (6, 10)]      # plain; the centre cell is singular for 'polar'; both poles sit on cell centres for 'bipolar'


def _direction_ref(alignment, angle_deg, H, W):
    """getCellDirection cell by cell in Python floats (float64): [2][H][W] lists, plane 0 = dir.x, plane 1 = dir.y"""
    a = math.radians(angle_deg)
    out = [[[0.0] * W for _ in range(H)] for _ in range(2)]
    for r in range(H):
        for q in range(W):
            x, y = q + 0.5, r + 0.5
            bx, by = 0.0, 1.0
            try:
                if alignment == "polar":
                    vx, vy = x - 0.5 * W, y - 0.5 * H
                    n = math.sqrt(vx * vx + vy * vy)
                    bx, by = vx / n, vy / n
                elif alignment == "bipolar":
                    v1 = (x - 0.25 * W, y - 0.25 * H)
                    v2 = (0.75 * W - x, 0.75 * H - y)
                    l1, l2 = math.sqrt(v1[0] ** 2 + v1[1] ** 2) ** 3, math.sqrt(v2[0] ** 2 + v2[1] ** 2) ** 3
                    vx, vy = v1[0] / l1 + v2[0] / l2, v1[1] / l1 + v2[1] / l2
                    n = math.sqrt(vx * vx + vy * vy)
                    bx, by = vx / n, vy / n
            except ZeroDivisionError:        # GLSL gives NaN here; the contract is (0, 1) before the rotation
                bx, by = 0.0, 1.0
            out[0][r][q] = math.cos(a) * bx - math.sin(a) * by
            out[1][r][q] = math.sin(a) * bx + math.cos(a) * by
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("angle", [0.0, 30.0, 200.0])
@pytest.mark.parametrize("alignment", ["cartesian", "polar", "bipolar"])
def test_direction_field_against_float64(alignment, angle, H, W):
    from ncahip import steer
    f = steer.direction_field(alignment, angle, H, W, "cpu")
    assert f.shape == (1, 2, H, W) and f.dtype == torch.float32 and f.is_contiguous()
    assert bool(torch.isfinite(f).all())
    ref = _direction_ref(alignment, angle, H, W)
    err = float((f[0].double() - ref).abs().max())
    norm = float(((f[0].double() ** 2).sum(0).sqrt() - 1.0).abs().max())
    print(f"{alignment} {angle} {H}x{W}: max |field - float64| {err:.2e} (float32 rounding: 6e-8), max | |dir| - 1 | {norm:.2e}")
    assert err <= 2.0 ** -23          # the float64 value rounded once to float32, components in [-1, 1]
    assert norm <= 1e-6
    if alignment == "cartesian" and angle == 0.0:
        assert torch.equal(f[0, 0], torch.zeros(H, W)) and torch.equal(f[0, 1], torch.ones(H, W))
    assert steer.direction_field(alignment, angle, H, W, "cpu") is f          # cached per (alignment, angle, H, W, device)


def test_singular_cells_take_the_cartesian_base():
    from ncahip import steer
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    f = steer.direction_field("polar", 30.0, 7, 9)
    assert abs(float(f[0, 0, 3, 4]) + s) < 1e-7 and abs(float(f[0, 1, 3, 4]) - c) < 1e-7          # rotate(30) * (0, 1) = (-sin, cos)
    f = steer.direction_field("bipolar", 30.0, 6, 10)
    for r, q in ((1, 2), (4, 7)):           # xy = 0.25 size and 0.75 size
        assert abs(float(f[0, 0, r, q]) + s) < 1e-7 and abs(float(f[0, 1, r, q]) - c) < 1e-7
    with pytest.raises(ValueError):
        steer.direction_field("hex", 0.0, 8, 8)


@pytest.mark.parametrize("angle", [0.0, 30.0, 200.0, -75.0])
def test_fold_angle_commutes_with_the_rotation(angle):
    """W1' y == W1 y' in float64 for random y: the unsteered step on folded weights is the uniformly steered step"""
    from ncahip import steer
    C, cc, fc, n = 5, 3, 11, 64
    g = torch.Generator().manual_seed(7)
    w1 = torch.randn(fc, 4 * C + cc, generator=g, dtype=torch.float64)
    y = torch.randn(1, 4 * C, 1, n, generator=g, dtype=torch.float64)
    cond = torch.randn(1, cc, 1, n, generator=g, dtype=torch.float64)
    a = math.radians(angle)
    sd, cd = -math.sin(a), math.cos(a)          # the uniform field of that angle: rotate(a) (0, 1), as direction_field('cartesian', angle)
    f32 = steer.direction_field("cartesian", angle, 1, n)
    assert abs(float(f32[0, 0, 0, 0]) - sd) < 1e-7 and abs(float(f32[0, 1, 0, 0]) - cd) < 1e-7
    dirs = torch.tensor([sd, cd], dtype=torch.float64).reshape(1, 2, 1, 1).expand(1, 2, 1, n)
    ys = steer.rotate_perception(y, dirs, C)
    # the two lines, restated: Sx' = c Sx - s Sy, Sy' = s Sx + c Sy
    assert torch.allclose(ys[:, C:2 * C], cd * y[:, C:2 * C] - sd * y[:, 2 * C:3 * C], rtol=0, atol=1e-15)
    assert torch.allclose(ys[:, 2 * C:3 * C], sd * y[:, C:2 * C] + cd * y[:, 2 * C:3 * C], rtol=0, atol=1e-15)
    assert torch.equal(ys[:, :C], y[:, :C]) and torch.equal(ys[:, 3 * C:], y[:, 3 * C:])
    w1f = steer.fold_angle(w1, C, angle)
    lhs = torch.einsum("jk,bkhw->bjhw", w1f, torch.cat((y, cond), 1))
    rhs = torch.einsum("jk,bkhw->bjhw", w1, torch.cat((ys, cond), 1))
    err = float((lhs - rhs).abs().max())
    print(f"angle {angle}: max |W1' y - W1 y'| {err:.2e}")
    assert err <= 1e-12
    assert steer.fold_angle(w1.reshape(fc, -1, 1, 1), C, angle).shape == (fc, 4 * C + cc, 1, 1)      # conv-shaped weights too
    if angle == 0.0:
        assert torch.equal(w1f, w1)


def test_rotate_pos_emb_at_90_degrees_swaps_the_planes():
    from ncahip import steer
    from ncahip.models.dynca import CPE2D
    emb = CPE2D()(torch.zeros(2, 4, 5, 7))
    assert torch.equal(emb[0, 0, :, 0], emb[0, 0, :, 3]) and torch.equal(emb[0, 1, 0], emb[0, 1, 2])      # emb[0]: along rows, emb[1]: along columns
    r = steer.rotate_pos_emb(emb, 90.0)          # s = 1, c = 0:  emb1' = emb0, emb0' = -emb1
    assert r.shape == emb.shape and torch.equal(r[:, 1], emb[:, 0]) and torch.equal(r[:, 0], -emb[:, 1])
    assert torch.equal(steer.rotate_pos_emb(emb, 0.0), emb)
    a = math.radians(30.0)
    r = steer.rotate_pos_emb(emb, 30.0)
    assert torch.allclose(r[:, 1], math.cos(a) * emb[:, 1] + math.sin(a) * emb[:, 0], atol=1e-6)
    assert torch.allclose(r[:, 0], -math.sin(a) * emb[:, 1] + math.cos(a) * emb[:, 0], atol=1e-6)


def test_c_entry_point_without_a_device():
    """ncahip_dynca_direction's own checks, and what an attached field makes the step entry points refuse -- all on the host"""
    from ncahip import _capi
    L = _capi.lib()
    one, two, fake = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)      # never dereferenced
    # a call the direction check is the only obstacle of until the fire-mask check refuses it (bit-packed masks with rate 1.5):
    # nothing below ever reaches a launch
    bits_seed = _capi.SEED_U_IS_BITS

    def step(H, W, B=1):
        return L.ncahip_dynca_step_fwd_f32(one, two, None, one, one, one, one, one, B, 12, H, W, 96, 0, 1, 1.5, bits_seed, 0, None)

    assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0
    try:
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
            assert L.ncahip_dynca_direction(fake, *bad) == _capi.EINVAL and b"direction" in L.ncahip_last_error()
        assert step(8, 12) == _capi.ERANGE and b"bit-packed" in L.ncahip_last_error()          # nothing attached by the refused calls
        assert L.ncahip_dynca_direction(fake, 1, 8, 8) == 0
        assert L.ncahip_dynca_direction(fake, 0, 8, 8) == _capi.EINVAL                          # ... and the attachment stays
        assert step(8, 12) == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        assert step(8, 8) == _capi.ERANGE and b"bit-packed" in L.ncahip_last_error()            # the field's own size passes
        assert step(8, 8, B=3) == _capi.ERANGE                                                  # Bd = 1 serves any batch
        # the other honouring entry points: the two-scale step, the persistent launch, the clip
        rc = L.ncahip_dynca_step_fwd_ms_f32(one, two, None, one, one, one, one, one, 1, 12, 8, 12, 96, 0, 1, 1.5, bits_seed, 0, one, None)
        assert rc == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        rc = L.ncahip_dynca_nsteps_fwd_persist_f32(one, two, 1, None, None, one, one, one, one, 1, 12, 16, 16, 96, 0, 1, 0.5, 0, 0,
                                                   ctypes.c_void_p(0x4000), 1 << 20, 1, None)
        assert rc == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        # entry points that do not steer refuse to run at all while a field is attached
        rc = L.ncahip_dynca_step_bwd_f32(one, None, None, one, one, one, one, 1, 12, 8, 8, 96, 0, 1, 0.5, 0, 0, one, two, one, one, one, None)
        assert rc == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        rc = L.ncahip_dynca_step_fwd_bf16(one, two, None, None, one, one, one, one, 1, 12, 8, 8, 96, 0, 1, 0.5, 0, 0, None)
        assert rc == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        need = L.ncahip_dynca_nsteps_bwd_workspace(1, 12, 8, 8, 96, 0)
        rc = L.ncahip_dynca_nsteps_bwd_f32(one, 1, None, None, one, one, one, one, 1, 12, 8, 8, 96, 0, 1, 0.5, 0, 0, one, None,
                                           two, one, one, one, one, ctypes.c_void_p(0x4000), need, None)
        assert rc == _capi.EINVAL and b"direction field" in L.ncahip_last_error()
        # a per-sample field: B must equal Bd
        assert L.ncahip_dynca_direction(fake, 2, 8, 8) == 0
        assert step(8, 8, B=3) == _capi.EINVAL and b"Bd = 2" in L.ncahip_last_error()
        assert step(8, 8, B=2) == _capi.ERANGE
    finally:
        assert L.ncahip_dynca_direction(None, 0, 0, 0) == 0
    assert step(8, 12) == _capi.ERANGE and b"bit-packed" in L.ncahip_last_error()               # detached: past that check again
    assert _capi.version() == 300


def test_ops_context_manager_validates_before_the_library():
    from ncahip import _capi, ops
    with pytest.raises(_capi.NcaHipError):
        with ops.dynca_direction(torch.zeros(1, 2, 8, 8)):          # a CPU tensor: no CPU fallback
            pass
    with pytest.raises(_capi.NcaHipError):
        with ops.dynca_direction(None):
            pass


@pytest.mark.parametrize("family", ["edges", "extra"])
def test_steered_step_refuses_autograd(family):
    """the recompute backward does not know the field: a steered call that would record a graph raises before anything runs"""
    if family == "edges":
        from ncahip.models.dynca import DyNCA
        m = DyNCA(12, 3, fc_dim=96, conditioning="edges", device=torch.device("cpu"))
        kw = {"cond_img": torch.zeros(1, 1, 8, 8)}
    else:
        from ncahip.models.dynca_extra import DyNCA
        m = DyNCA(13, 3, fc_dim=96, device=torch.device("cpu"))
        kw = {}
    x = torch.zeros(1, m.c_in, 8, 8)
    with pytest.raises(ValueError, match="inference only"):
        m.forward_nsteps(x, 2, direction=("polar", 30.0), **kw)
    with pytest.raises(ValueError, match="inference only"):
        m.forward(x, direction=torch.zeros(1, 2, 8, 8), **kw)
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="inference only"):
        m.forward_nsteps(x.clone().requires_grad_(True), 2, direction=("cartesian", 0.0), **kw)
    # and a malformed direction is a ValueError too, not a kernel's problem
    with torch.no_grad():
        with pytest.raises(ValueError, match="direction"):
            m.forward_nsteps(x, 2, direction=torch.zeros(1, 2, 8, 9), **kw)
        with pytest.raises(ValueError, match="alignment"):
            m.forward_nsteps(x, 2, direction=("spiral", 0.0), **kw)
