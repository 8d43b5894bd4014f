"""GPU tests of the cells of the emit launcher (nca_launch_clip_emit, csrc/nca_clip.hip) that no other module reaches: a uint8 image at
a pointer that is not 4-byte aligned (ops allocates aligned images, so every other test takes the kernel's aligned stores) for every
kind of call -- image, image + grey plane, ConditionedNCA's image of an fp32 and of a bf16 state -- and the planar image of a bf16
state at such a pointer.  The smallest shapes that still take the launcher's branches: uint8 at 2 x 3 x 5 (30 pixels: seven groups of
four and a partial one), planar at 6 x 10 (the last column block holds two pixels), inject at C = 5, c_out = 3.  Every comparison is
torch.equal; the bytes around the image stay untouched."""
import pytest
import torch

from gpu_ops import gpu_ops
from test_gpu_clip_yuv_out import P, guarded, guards_intact, layout_word

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = 1


@pytest.fixture(scope="module")
def ops():
    with gpu_ops(persistent_steps=True) as o:
        yield o
        o.check_errors()


def _state(B, C, H, W, seed):
    x = torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed)) * 2.4 - 1.2      # beyond both ends of both images' ranges
    x.view(-1)[:6] = torch.tensor([0.5, -0.5, 0.0, 1.0, 3.0, -3.0])
    return x.to(DEV)


def _u8(img):
    """float image [B,c,H,W] in [0, 1] -> the truncated uint8 image [B,H,W,c]"""
    return (img * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("entry", ["emit c_out=1", "emit c_out=2", "emit c_out=3", "emit c_out=4", "emit_inject", "emit_unit", "emit_unit_bf16"])
def test_uint8_image_at_an_odd_pointer(ops, entry):
    B, C, H, W = 2, 5, 3, 5
    L, st = ops.lib(), ops._stream()
    x = _state(B, C, H, W, 5)
    c_out = int(entry[-1]) if entry.startswith("emit c_out") else 3
    nbytes = B * H * W * c_out
    buf, img = guarded(nbytes, 1)
    assert img.data_ptr() % 4 == 1
    if entry.startswith("emit_unit"):
        if entry == "emit_unit_bf16":
            x = x.bfloat16()
            rc = L.ncahip_clip_emit_unit_bf16(P(x), P(img), U8, B, C, H, W, st)
        else:
            rc = L.ncahip_clip_emit_unit(P(x), P(img), U8, B, C, H, W, st)
        want = _u8(x[:, :3].float().clamp(0, 1))
    elif entry == "emit_inject":
        gray = torch.rand(B, H, W, generator=torch.Generator().manual_seed(6)).to(DEV) * 2 - 1
        s = x.clone()
        rc = L.ncahip_clip_emit_inject(P(s), P(img), U8, P(gray), B, C, c_out, H, W, st)
        assert torch.equal(s[:, :C - 1], x[:, :C - 1]) and torch.equal(s[:, C - 1], gray)
        want = _u8((2 * x[:, :c_out]).clamp(-1, 1).add(1).div(2))
    else:
        rc = L.ncahip_clip_emit(P(x), P(img), U8, B, C, c_out, H, W, st)
        want = _u8((2 * x[:, :c_out]).clamp(-1, 1).add(1).div(2))
    assert rc == 0, L.ncahip_last_error()
    assert torch.equal(img.view(B, H, W, c_out), want), entry
    assert guards_intact(buf, 1, nbytes), entry
    assert int(want.min()) == 0 and int(want.max()) == 255


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_planar_image_of_a_bf16_state_at_an_odd_pointer(ops, fmt):
    """against the planar image of the widened state, which test_gpu_clip_yuv_out.py holds to the uint8 image and the conversion"""
    B, C, H, W = 2, 4, 6, 10
    L, st = ops.lib(), ops._stream()
    x = _state(B, C, H, W, 7).bfloat16()
    want = ops.clip_emit_unit(x.float(), torch.uint8, fmt, "bt601", "full")
    nbytes = B * H * W * 3 // 2
    for off in (1, 2, 3):
        buf, img = guarded(nbytes, off)
        assert L.ncahip_clip_emit_unit_bf16(P(x), P(img), layout_word(ops, fmt, ("bt601", "full")), B, C, H, W, st) == 0, L.ncahip_last_error()
        assert torch.equal(img.view(B, 3 * H // 2, W), want), (fmt, off)
        assert guards_intact(buf, off, nbytes), (fmt, off)
