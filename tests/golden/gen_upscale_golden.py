#!/usr/bin/env python3
"""Generate tests/golden/g13_clip_upscale.npz with Pillow alone: small uint8 images at model-grid sizes, a case list and what Pillow's
8-bit Image.resize returns when it brings each of them to a delivery size (enlarging, mostly).  No project code runs here.

    python tests/golden/gen_upscale_golden.py

The whole image is resized (no crop), as out_size= of the clip calls does.  The file holds:
    in_<i>        uint8 [H,W,3]          the inputs (none larger than 24 x 32)
    case_input    int32 [n]              index of the input
    case_size     int32 [n,2]            (out_h, out_w), the delivery size -- both even, so that the planar formats apply
    case_filter   str   [n]              'bicubic' or 'lanczos'
    out_<c>       uint8 [out_h,out_w,3]  Pillow's result of case c
    pillow        str                    the Pillow version that wrote the file
"""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g13_clip_upscale.npz")
FILTERS = {"bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def main():
    rng = np.random.default_rng(13)
    checker = np.zeros((16, 24, 3), dtype=np.uint8)
    checker[(np.add.outer(np.arange(16), np.arange(24)) % 2) == 1] = 255
    inputs = [rng.integers(0, 256, (10, 14, 3), dtype=np.uint8),          # 0: non-integer ratios, out_w % 4 == 2
              rng.integers(0, 256, (16, 24, 3), dtype=np.uint8),          # 1: the host tests' grid
              rng.integers(0, 256, (9, 7, 3), dtype=np.uint8),            # 2: odd grid, exact 2 x
              rng.integers(0, 256, (20, 24, 3), dtype=np.uint8),          # 3: identity
              rng.integers(0, 256, (4, 6, 3), dtype=np.uint8),            # 4: a 6 x 6 planar image (V plane at byte 45)
              checker]                                                   # 5: 0 / 255 checkerboard: overshoot, both clamps
    cases = []                                                           # (input, (out_h, out_w), filter)
    for filt in FILTERS:
        cases += [(0, (22, 30), filt), (2, (18, 14), filt), (4, (6, 6), filt)]
    cases += [(1, (36, 52), "lanczos"), (5, (36, 52), "bicubic"), (3, (20, 24), "lanczos")]
    data = {f"in_{i}": a for i, a in enumerate(inputs)}
    for c, (i, size, filt) in enumerate(cases):
        out = np.asarray(Image.fromarray(inputs[i]).resize((size[1], size[0]), FILTERS[filt]))      # Pillow takes (x, y)
        assert out.shape == (size[0], size[1], 3) and out.dtype == np.uint8
        data[f"out_{c}"] = out
    data["case_input"] = np.array([c[0] for c in cases], dtype=np.int32)
    data["case_size"] = np.array([c[1] for c in cases], dtype=np.int32)
    data["case_filter"] = np.array([c[2] for c in cases])
    data["pillow"] = np.array(PIL.__version__)
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes, Pillow {PIL.__version__}")
    assert os.path.getsize(OUT) < 32 * 1024


if __name__ == "__main__":
    main()
