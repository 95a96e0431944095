#!/usr/bin/env python3
"""Write tests/golden/mjpeg_sync/*.jpg: small 4:2:0 baseline JPEG files coded by Pillow (libjpeg) for the self-synchronising entropy
decoder (include/hv_mjpeg_sync.h; tests/test_mjpeg_sync_cpu.py, tests/test_gpu_mjpeg_sync.py, tools/mjpeg_sync_check.cpp), without
restart markers unless noted: what the algorithm distinguishes must occur in them (the census of tests/test_mjpeg_sync_cpu.py).
    noise_64x48_q100_s0    quality 100, default_rng(0): 6063 scan bytes = 379 subsequences of 16 bytes, two rounds, FF 00 pairs
                           that straddle a subsequence edge
    noise_64x48_q100_s2    seed 2: 6064 scan bytes, an exact multiple of 16
    noise_64x48_q95opt_s2  quality 95, optimize=True, seed 2: 3121 scan bytes, Pillow's own Huffman tables
    flat_64x48             all 128: 48 scan bytes, about twenty blocks per subsequence
    ramp_80x64_q75         a smooth ramp: 440 scan bytes
    one_1x1                8 scan bytes, less than one subsequence
    ri3_37x53_q75          restart markers every 3 MCUs, which at 37 pixels is one MCU row, as the reader's fixtures have them
    rows1_53x37_q75        restart markers every MCU row of 4 MCUs (Ri = 4)
The files are committed: another Pillow may code other bytes (the sizes below are asserted so that this is noticed).
Run:  python tools/make_golden_mjpeg_sync.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mjpeg_sync")


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def ramp(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([255 * x / (W - 1), 255 * y / (H - 1), 255 * (x + y) / (W + H - 2)], -1).astype(np.uint8)


def encode(arr, quality=75, **kw):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, "JPEG", quality=quality, subsampling=2, **kw)
    return b.getvalue()


def scan_bytes(d):
    """the entropy-coded bytes between the SOS segment and EOI"""
    pos = 2
    while d[pos + 1] != 0xDA:
        pos += 2 + d[pos + 2] * 256 + d[pos + 3]
    return len(d) - 2 - (pos + 2 + d[pos + 2] * 256 + d[pos + 3])


# (file name, image, Pillow's save arguments, scan bytes or None)
CASES = (("noise_64x48_q100_s0.jpg", noise(64, 48, 0), dict(quality=100), 6063),
         ("noise_64x48_q100_s2.jpg", noise(64, 48, 2), dict(quality=100), 6064),
         ("noise_64x48_q95opt_s2.jpg", noise(64, 48, 2), dict(quality=95, optimize=True), 3121),
         ("flat_64x48.jpg", np.full((48, 64, 3), 128, np.uint8), dict(), 48),
         ("ramp_80x64_q75.jpg", ramp(80, 64), dict(quality=75), 440),
         ("one_1x1.jpg", noise(1, 1, 1), dict(), 8),
         ("ri3_37x53_q75.jpg", noise(37, 53, 37053), dict(quality=75, restart_marker_blocks=3), None),
         ("rows1_53x37_q75.jpg", noise(53, 37, 53037), dict(quality=75, restart_marker_rows=1), None))

if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for fname, arr, kw, want in CASES:
        data = encode(arr, **kw)
        n = scan_bytes(data)
        print(f"{fname}: {len(data)} bytes, {n} of them the scan")
        assert want is None or n == want, f"{fname}: {n} scan bytes, expected {want} (another Pillow?)"
        with open(os.path.join(OUT, fname), "wb") as f:
            f.write(data)
    sys.exit(0)
