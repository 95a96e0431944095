#!/usr/bin/env python3
"""Generate tests/golden/metrics_frames.npz by EXECUTING the reference's compute_psnr / compute_ssim (evaluation/compute_metrics.py)
on a fixed list of uint8 frame pairs.

The reference file is loaded by path; its imports that are absent here (lpips, imageio, tqdm, and torch where the interpreter has
none) are stubbed in memory - neither function touches them.  It needs an interpreter with scikit-image; 0.18.3 predates
`channel_axis`, so `structural_similarity` is wrapped to translate `channel_axis=-1` into `multichannel=True` (same arithmetic), and the
skimage version is stored in the npz.  numpy only otherwise.

Every pair is stored as fp16 tensors in [-1, 1] ([C,H,W], exactly representable in fp16, so fp16 and fp32 inputs of a test hold the
same values), the uint8 bytes save_videos_grid(..., rescale=True) makes of them (stored [C,H,W] like the tensors: it compresses better; computed here with the reference's own
three fp32 steps) and the two scores.  A reference frame is stored once per (size, content) and shared by its distortions.
Run:  <python with scikit-image> tools/make_golden_metrics.py <reference root>"""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "metrics_frames.npz")

# (H, W, C, content, [distortions]); content: random | ramp | narrow | const; distortion: none | pm1 | pm9 | pm60 | inv | const
ALL = ["none", "pm1", "pm9", "pm60", "inv"]
CASES = [
    (7, 7, 3, "random", ALL), (7, 7, 3, "ramp", ALL), (7, 7, 3, "narrow", ALL),
    (7, 40, 3, "random", ALL), (7, 40, 3, "ramp", ALL), (7, 40, 3, "narrow", ALL),
    (24, 31, 3, "random", ALL + ["const"]), (24, 31, 3, "ramp", ["pm9"]), (24, 31, 3, "narrow", ["pm1"]),
    (24, 31, 3, "const", ["pm9"]), (24, 31, 1, "random", ["pm9"]),
    (45, 80, 3, "random", ["pm9"]), (45, 80, 3, "ramp", ["inv"]),
    (33, 257, 3, "narrow", ["pm1"]),
    (90, 160, 3, "ramp", ["pm60"]),
]


def load_reference(ref_root):
    import skimage
    import skimage.metrics as skm
    noop = types.SimpleNamespace
    for name in ("lpips", "imageio", "tqdm", "torch"):
        try:
            __import__(name)
        except ImportError:
            m = types.ModuleType(name)
            m.tqdm = lambda it, **k: it
            sys.modules[name] = m
    orig = skm.structural_similarity
    if "channel_axis" not in orig.__code__.co_varnames:
        def structural_similarity(im1, im2, *, channel_axis=None, **kw):
            assert channel_axis in (None, -1)
            return orig(im1, im2, multichannel=channel_axis == -1, **kw)
        skm.structural_similarity = structural_similarity
    spec = importlib.util.spec_from_file_location("ref_compute_metrics", os.path.join(ref_root, "evaluation", "compute_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    del noop
    return mod, skimage.__version__


def content(rng, kind, H, W, C):
    if kind == "random":
        return rng.integers(0, 256, (H, W, C), dtype=np.int64)
    if kind == "narrow":
        return rng.integers(100, 104, (H, W, C), dtype=np.int64)
    if kind == "const":
        return np.full((H, W, C), 77, dtype=np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = [(20 + 200 * xx / max(W - 1, 1)), (230 - 190 * yy / max(H - 1, 1)), (40 + 90 * (xx + yy) / max(H + W - 2, 1))]
    return np.stack([ramp[c % 3] for c in range(C)], axis=-1).astype(np.int64)


def distort(rng, q, kind):
    if kind == "none":
        return q.copy()
    if kind == "inv":
        return 255 - q
    if kind == "const":
        return np.full_like(q, 200)
    d = int(kind[2:])
    return np.clip(q + d * rng.choice([-1, 1], q.shape), 0, 255)


def to_float(rng, q, jitter):
    """fp16 values in [-1, 1] that quantise to the bytes q: somewhere inside the byte's bin (jitter) or at its centre"""
    frac = rng.uniform(0.1, 0.9, q.shape) if jitter else 0.5
    return ((q + frac) / 255.0 * 2.0 - 1.0).astype(np.float16).transpose(2, 0, 1)


def frames_bytes(x_chw):
    """save_videos_grid(rescale=True) on one frame: (x + 1.0) / 2.0, clamp(0, 1), * 255 in fp32, astype(uint8)"""
    x = x_chw.astype(np.float32).transpose(1, 2, 0)
    x = (x + np.float32(1.0)) / np.float32(2.0)
    return (np.clip(x, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_metrics.py <root of the reference checkout>")
    ref_root = sys.argv[1]
    mod, version = load_reference(ref_root)
    rng = np.random.default_rng(20240607)
    out, names = {}, []
    for H, W, C, kind, dists in CASES:
        q1 = content(rng, kind, H, W, C)
        jitter = kind == "random" and H * W <= 24 * 31
        x1 = to_float(rng, q1, jitter)
        b1 = frames_bytes(x1)
        assert np.array_equal(b1, q1.astype(np.uint8)), (H, W, kind)
        rkey = f"{H}x{W}x{C}_{kind}"
        out[f"ref_{rkey}"] = x1
        out[f"refbytes_{rkey}"] = np.ascontiguousarray(b1.transpose(2, 0, 1))
        for d in dists:
            q2 = distort(rng, q1, d)
            x2 = to_float(rng, q2, jitter)
            b2 = frames_bytes(x2)
            assert np.array_equal(b2, q2.astype(np.uint8)), (H, W, kind, d)
            name = f"{rkey}_{d}"
            names.append(name)
            out[f"rec_{name}"] = x2
            out[f"recbytes_{name}"] = np.ascontiguousarray(b2.transpose(2, 0, 1))
            out[f"psnr_{name}"] = np.float64(mod.compute_psnr(b1, b2))
            out[f"ssim_{name}"] = np.float64(mod.compute_ssim(b1, b2))
            print(f"{name:28s} psnr {float(out['psnr_' + name]):10.5f}  ssim {float(out['ssim_' + name]):+.9f}")
    out["names"] = np.array(names)
    out["skimage_version"] = np.array(version)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(names)} pairs, {os.path.getsize(OUT)} bytes, skimage {version}")


if __name__ == "__main__":
    main()
