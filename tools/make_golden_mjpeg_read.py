#!/usr/bin/env python3
"""Write tests/golden/mjpeg_read/*.jpg: small 4:2:0 baseline JPEG files coded by Pillow (libjpeg), the foreign inputs of the decoder tests
(tests/test_mjpeg_read_cpu.py compares the restatement with Pillow's decode on them, tests/test_gpu_mjpeg_read.py decodes them on the
GPU without Pillow, tools/mjpeg_decode_fuzz.cpp mutates them).  Seeded noise at 37 x 53 and 5 x 4; plain tables, optimised tables, a
restart interval of 3 MCUs and of one MCU row; quality 35, 75 and 95.  At 37 x 53 an MCU row IS 3 MCUs, so ri3_37x53_* and
rows1_37x53_* are the same bytes (both kept: they are the cases the tests name), and at 5 x 4 there is one MCU.  Intervals that do not
line up with MCU rows come from two more kinds: ri3_53x37_* (4 x 3 MCUs, Ri = 3: four intervals, three of which begin inside a row and
span two rows) and ri5_37x53_* (3 x 4 MCUs, Ri = 5: intervals of 5, 5 and 2 MCUs, each crossing rows, the last one shorter).  The files
are committed: another Pillow may code other bytes, the tests only need some valid files of each kind.
Run:  python tools/make_golden_mjpeg_read.py"""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mjpeg_read")
SIZES = ((37, 53), (5, 4))
QUALITIES = (35, 75, 95)
VARIANTS = {"plain": {}, "optimize": {"optimize": True}, "ri3": {"restart_marker_blocks": 3}, "rows1": {"restart_marker_rows": 1}}


def image(W, H):
    return np.random.default_rng(1000 * W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)


def encode(arr, quality, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", quality=quality, subsampling=2, **kw)
    return b.getvalue()


# restart intervals that cross MCU rows: (name, W, H, Pillow's save arguments, Ri, intervals per frame)
CROSSING = (("ri3", 53, 37, {"restart_marker_blocks": 3}, 3, 4), ("ri5", 37, 53, {"restart_marker_blocks": 5}, 5, 3))


def cases():
    """(file name, W, H, quality, Pillow's save arguments)"""
    return [(f"{name}_{W}x{H}_q{q}.jpg", W, H, q, kw) for W, H in SIZES for q in QUALITIES for name, kw in VARIANTS.items()] + \
        [(f"{name}_{W}x{H}_q{q}.jpg", W, H, q, kw) for name, W, H, kw, _, _ in CROSSING for q in QUALITIES]


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for fname, W, H, q, kw in cases():
        data = encode(image(W, H), q, **kw)
        with open(os.path.join(OUT, fname), "wb") as f:
            f.write(data)
        print(f"{fname}: {len(data)} bytes")
