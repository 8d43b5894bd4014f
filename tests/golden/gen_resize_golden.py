#!/usr/bin/env python3
"""Generate tests/golden/g12_clip_resize.npz with Pillow alone: small uint8 frames, a case list and what Pillow's 8-bit Image.resize
returns for each case after the reference's crop.  No project code runs here.

    python tests/golden/gen_resize_golden.py

The two reference paths (EncoderConditioning/utils/utils.py:5-25 and ConditioneDyNCA/utils/misc/preprocess_texture.py:9-33) are restated
as `_crop_box`; the crop is applied the way each of them does it (Image.crop / numpy slicing), then Image.resize runs with the filter
named in the case.  The file holds:
    in_<i>        uint8 [H,W,3]          the inputs (none larger than 45 x 80)
    case_input    int32 [n]              index of the input
    case_crop     str   [n]              'none', 'dynca', 'conditioned' or 'box'
    case_box      int32 [n,4]            the crop as (x0, y0, w, h)
    case_size     int32 [n,2]            (out_h, out_w)
    case_filter   str   [n]              'bicubic' or 'lanczos'
    out_<c>       uint8 [out_h,out_w,3]  Pillow's result of case c
    pillow        str                    the Pillow version that wrote the file
"""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g12_clip_resize.npz")
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def _crop_box(kind, H, W):
    if kind == "none":
        return 0, 0, W, H
    if kind == "dynca":                      # preprocess_texture.py:17-25
        cut = abs(W - H) // 2
        return (cut, 0, W - 2 * cut, H) if W > H else (0, cut, W, H - 2 * cut)
    n = min(W, H)                            # utils.py:10-16
    left, top = (W - n) // 2, (H - n) // 2
    return left, top, (W + n) // 2 - left, (H + n) // 2 - top


def _resize(img, kind, box, size, filt):
    x0, y0, w, h = box
    if kind == "conditioned":
        pil = Image.fromarray(img).crop((x0, y0, x0 + w, y0 + h))
    else:
        pil = Image.fromarray(np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]))
    out = np.asarray(pil.resize((size[1], size[0]), FILTERS[filt]))          # Pillow takes (x, y)
    assert out.shape == (size[0], size[1], 3) and out.dtype == np.uint8
    return out


def main():
    rng = np.random.default_rng(12)
    checker = np.zeros((16, 16, 3), dtype=np.uint8)
    checker[(np.add.outer(np.arange(16), np.arange(16)) % 2) == 1] = 255
    smooth = np.clip(np.add.outer(np.arange(33) * 7.0, np.arange(21) * 5.0)[..., None] + np.array([0.0, 40.0, 90.0]), 0, 255).astype(np.uint8)
    inputs = [rng.integers(0, 256, (45, 80, 3), dtype=np.uint8),          # 0: a 16:9 frame, odd height
              rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),          # 1: odd both ways
              rng.integers(0, 256, (20, 24, 3), dtype=np.uint8),          # 2: for upscaling
              smooth,                                                    # 3: a 33 x 21 ramp (portrait)
              checker,                                                   # 4: 0 / 255 checkerboard: both clamps
              np.full((1, 1, 3), 200, dtype=np.uint8),                   # 5: a single pixel
              (rng.integers(0, 2, (12, 31, 3)) * 255).astype(np.uint8)]   # 6: saturated noise
    cases = []                                                           # (input, crop kind or box, (out_h, out_w), filter)
    for filt in FILTERS:
        cases += [(0, "dynca", (16, 16), filt), (0, "conditioned", (16, 16), filt), (0, "none", (9, 16), filt),
                  (0, (3, 1, 31, 29), (12, 10), filt), (1, "dynca", (16, 16), filt), (1, "conditioned", (8, 12), filt),
                  (2, "none", (40, 48), filt), (3, "dynca", (16, 32), filt), (3, "conditioned", (7, 7), filt),
                  (4, "none", (11, 13), filt), (4, "none", (16, 16), filt), (4, "none", (24, 20), filt),
                  (5, "none", (4, 4), filt), (6, "conditioned", (5, 9), filt), (1, "none", (1, 1), filt), (1, "none", (3, 2), filt)]
    data = {f"in_{i}": a for i, a in enumerate(inputs)}
    boxes, kinds = [], []
    for c, (i, crop, size, filt) in enumerate(cases):
        H, W = inputs[i].shape[:2]
        kind = crop if isinstance(crop, str) else "box"
        box = _crop_box(kind, H, W) if isinstance(crop, str) else crop
        data[f"out_{c}"] = _resize(inputs[i], kind, box, size, filt)
        boxes.append(box)
        kinds.append(kind)
    data["case_input"] = np.array([c[0] for c in cases], dtype=np.int32)
    data["case_crop"] = np.array(kinds)
    data["case_box"] = np.array(boxes, dtype=np.int32)
    data["case_size"] = np.array([c[2] for c in cases], dtype=np.int32)
    data["case_filter"] = np.array([c[3] for c in cases])
    data["pillow"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes, Pillow {PIL.__version__}")
    assert os.path.getsize(OUT) < 64 * 1024


if __name__ == "__main__":
    main()
