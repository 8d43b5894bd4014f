"""Steering a trained DyNCA at run time (the WebGL runtime's `rotationAngle` / `alignment`, docs/dynca.js:209-225, :417-426, :569-577).

A direction field is dirs [Bd,2,H,W] float32, plane 0 = s, plane 1 = c (dir.x, dir.y of dynca.js:420-421).  The fused step kernels
rotate every cell's Sobel pair by it (ops.dynca_direction, ncahip_dynca_direction in include/ncahip.h):

    Sx' = c Sx - s Sy        Sy' = s Sx + c Sy        (x and the Laplacian untouched)

on the FINAL perception -- two-scale: after the blend with the up-sampled coarse level.  The WebGL runtime rotates each scale at its own
resolution; the rotation is linear, so for a uniform field the two definitions agree exactly, and for a varying field they differ on
the coarse half.

Everything here is host-side torch and small:
  direction_field   getCellDirection restated: 'cartesian', 'polar' or 'bipolar' plus a global angle -> the field
  fold_angle        a UNIFORM angle needs no field and no kernel: it folds into w1's Sobel columns.  That is the cheaper route for a
                    global angle; the field path exists for directions that vary over the grid
  rotate_pos_emb    the positional encoding of a pos_emb model turned by the same angle (dynca.js:569-577)
  rotate_perception the two lines above in torch, for the composed multi-scale step
"""
import math

import torch

ALIGNMENTS = ("cartesian", "polar", "bipolar")      # u_alignment 0, 1, 2 of dynca.js:214-222

_FIELDS = {}


def _cos_sin(angle_deg: float):
    """(cos, sin) of an angle in degrees as Python floats; what rounds to a multiple of 90 degrees is exact (90: (0, 1))."""
    a = math.radians(float(angle_deg))
    c, s = math.cos(a), math.sin(a)
    return (0.0 if abs(c) < 1e-15 else c), (0.0 if abs(s) < 1e-15 else s)


def direction_field(alignment: str, angle_deg: float, H: int, W: int, device="cpu") -> torch.Tensor:
    """getCellDirection (dynca.js:209-225) for every cell of an H x W grid: float32 [1,2,H,W], plane 0 = dir.x = s, plane 1 = dir.y = c.

    xy = (col + 0.5, row + 0.5), size = (W, H).  The base direction is (0, 1) for 'cartesian', normalize(xy - 0.5 size) for 'polar',
    normalize(v1 / |v1|^3 + v2 / |v2|^3) with v1 = xy - 0.25 size, v2 = 0.75 size - xy for 'bipolar'; it is then rotated by
    [[cos a, -sin a], [sin a, cos a]].  A cell whose base is not finite -- the exact centre for odd H and W, the two poles for
    H, W = 2 (mod 4); GLSL gives NaN there -- takes (0, 1) before the rotation.  Computed in float64; cached per
    (alignment, angle, H, W, device): treat the result as read-only."""
    if alignment not in ALIGNMENTS:
        raise ValueError(f"alignment must be one of {ALIGNMENTS}, got {alignment!r}")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"direction_field: the grid must be at least 1 x 1, got {H} x {W}")
    dev = torch.device(device)
    key = (alignment, float(angle_deg), H, W, str(dev))
    hit = _FIELDS.get(key)
    if hit is not None:
        return hit
    x = (torch.arange(W, dtype=torch.float64) + 0.5)[None, :].expand(H, W)
    y = (torch.arange(H, dtype=torch.float64) + 0.5)[:, None].expand(H, W)
    if alignment == "cartesian":
        bx, by = torch.zeros(H, W, dtype=torch.float64), torch.ones(H, W, dtype=torch.float64)
    else:
        if alignment == "polar":
            vx, vy = x - 0.5 * W, y - 0.5 * H
        else:
            v1x, v1y, v2x, v2y = x - 0.25 * W, y - 0.25 * H, 0.75 * W - x, 0.75 * H - y
            n1, n2 = torch.hypot(v1x, v1y) ** 3, torch.hypot(v2x, v2y) ** 3
            vx, vy = v1x / n1 + v2x / n2, v1y / n1 + v2y / n2
        n = torch.hypot(vx, vy)
        bx, by = vx / n, vy / n
        bad = ~(torch.isfinite(bx) & torch.isfinite(by))
        bx, by = torch.where(bad, torch.zeros_like(bx), bx), torch.where(bad, torch.ones_like(by), by)
    c, s = _cos_sin(angle_deg)
    field = torch.stack((c * bx - s * by, s * bx + c * by))[None].to(torch.float32).contiguous().to(dev)
    if len(_FIELDS) >= 64:      # a handful of (alignment, angle, size) per run is the use; an angle sweep must not grow without bound
        _FIELDS.clear()
    _FIELDS[key] = field
    return field


def fold_angle(w1: torch.Tensor, c_in: int, angle_deg: float) -> torch.Tensor:
    """w1 [fc, 4 c_in + c_cond(, 1, 1)] with the UNIFORM field direction_field('cartesian', angle_deg, ...) folded into its Sobel columns.
    With (s, c) that field's direction -- rotate(angle) (0, 1) = (-sin angle, cos angle) in every cell --

        W1'[:, Sx] = c W1[:, Sx] + s W1[:, Sy]        W1'[:, Sy] = -s W1[:, Sx] + c W1[:, Sy]

    so that W1' y == W1 y' for the steered perception y' of every cell -- the unsteered kernels on W1' compute the steered step.  This
    is the cheaper route for a global angle (no field, no extra work per step); a direction that varies over the grid needs the field."""
    cos_a, sin_a = _cos_sin(angle_deg)
    c, s = cos_a, -sin_a
    C = int(c_in)
    out = w1.detach().clone()
    sx, sy = w1.detach()[:, C:2 * C], w1.detach()[:, 2 * C:3 * C]
    out[:, C:2 * C] = c * sx + s * sy
    out[:, 2 * C:3 * C] = -s * sx + c * sy
    return out


def rotate_pos_emb(emb: torch.Tensor, angle_deg: float) -> torch.Tensor:
    """CPE2D's output [..., 2, H, W] (emb[0] varies along rows, emb[1] along columns) turned as the WebGL runtime turns its positional
    encoding (pemb = rotate(-angle) * pemb, dynca.js:569-577):  emb1' = c emb1 + s emb0,  emb0' = -s emb1 + c emb0."""
    c, s = _cos_sin(angle_deg)
    e0, e1 = emb.select(-3, 0), emb.select(-3, 1)
    return torch.stack((-s * e1 + c * e0, c * e1 + s * e0), dim=-3).contiguous()


def rotate_perception(y: torch.Tensor, dirs: torch.Tensor, c_in: int) -> torch.Tensor:
    """The kernels' two lines in torch: y [B, 4 c_in, H, W] = [x | Sx | Sy | L] (no conditioning rows yet), dirs [Bd,2,H,W]."""
    C = int(c_in)
    s, c = dirs[:, 0:1].to(y.dtype), dirs[:, 1:2].to(y.dtype)
    sx, sy = y[:, C:2 * C], y[:, 2 * C:3 * C]
    return torch.cat((y[:, :C], c * sx - s * sy, s * sx + c * sy, y[:, 3 * C:]), dim=1)


def resolve(direction, H: int, W: int, device):
    """direction as the models take it -- a field tensor [Bd,2,H,W] or an (alignment, angle_deg) tuple -> (field float32 [Bd,2,H,W] on
    `device`, angle_deg or None).  The angle is returned for a tuple only: a pos_emb model turns its encoding by it."""
    if isinstance(direction, torch.Tensor):
        if direction.dim() != 4 or direction.shape[1] != 2 or tuple(direction.shape[2:]) != (int(H), int(W)):
            raise ValueError(f"direction field must be [Bd,2,{int(H)},{int(W)}], got {tuple(direction.shape)}")
        return direction.to(device=device, dtype=torch.float32).contiguous(), None
    try:
        alignment, angle = direction
    except (TypeError, ValueError):
        raise ValueError(f"direction must be a field tensor [Bd,2,H,W] or an (alignment, angle_deg) tuple, got {direction!r}") from None
    return direction_field(alignment, float(angle), H, W, device), float(angle)
