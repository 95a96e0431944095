#!/usr/bin/env python3
"""Time the Gaussian-window SSIM kernel (csrc/hv_gssim.hip) with HIP events: warm-up, then --reps timed windows of --inner launches
each, median per launch.  Two shapes - a 129-frame 720p fp16 clip and a 33-frame 240 x 416 fp16 clip - in both modes (temporal = 1: the
window over T, H, W; temporal = 0: over H, W), outputs and workspace allocated beforehand.

Per case: `ms` of hv_gaussian_ssim (kernel + fold), `positions` = map positions, `fma` = 165 (110 without the T axis) multiply-adds per
position as the definition counts them and `fp64_TFMAps` = fma / ms, `hbm_bytes` = what the algorithm must move (both clips once, the sums)
and `GBps`; for comparison in the same call `torch_fp32_ms`: torch's grouped-conv3d formulation of the same score in fp32 on the same card
(pytorch_msssim's own arithmetic; fields through HBM; its peak memory is why the 720p case runs it on frame chunks with a 10-frame overlap),
with `torch_fp32_mean_diff`, its distance from the kernel's mean; and `host_numpy_s`: numpy float64 on this machine's CPU from the 8-bit
codes, the copy included (one repetition, on the first --host-frames output frames and scaled to the clip; --no-host skips it).

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("720p129f", (3, 129, 720, 1280)), ("240p33f", (3, 33, 240, 416)))
WIN = 11


def timed(fn, warmup, reps, inner):
    """median / min / max ms of ONE call of fn, from `reps` event windows of `inner` calls each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def torch_sum(a, b, win32, temporal, chunk):
    """sum of the SSIM map by grouped conv3d in fp32 (pytorch_msssim's arithmetic) on [C,T,H,W] fp16 in [-1, 1]; `chunk` output frames
    at a time"""
    C, T = a.shape[:2]
    w = win32.view(1, 1, 1, 1, -1).repeat(C, 1, 1, 1, 1)

    def gf(x):
        for i in range(3):
            if i > 0 or temporal:
                x = F.conv3d(x, w.transpose(2 + i, -1), groups=C)
        return x
    total = torch.zeros((), dtype=torch.float64, device=a.device)
    To = T - (WIN - 1) * temporal
    for t0 in range(0, To, chunk):
        t1 = min(To, t0 + chunk) + (WIN - 1) * temporal
        q = lambda v: torch.floor(((v[:, t0:t1].float() + 1.0) * 0.5).clamp(0.0, 1.0) * 255.0)[None] / 255.0     # noqa: E731
        X, Y = q(a), q(b)
        m1, m2 = gf(X), gf(Y)
        s1, s2, s12 = gf(X * X) - m1 * m1, gf(Y * Y) - m2 * m2, gf(X * Y) - m1 * m2
        m = ((2 * m1 * m2 + 1e-4) / (m1 * m1 + m2 * m2 + 1e-4)) * ((2 * s12 + 9e-4) / (s1 + s2 + 9e-4))
        total += m.double().sum()
    return total


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--host-frames", type=int, default=2)
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    from hunyuanvideo_efficiency_amd import _lib, metrics
    from tests import gssim_ref, metrics_ref
    dev = "cuda:0"
    out = []
    for label, shape in SHAPES:
        C, T, H, W = shape
        g = torch.Generator(device=dev).manual_seed(0)
        x = (torch.rand(shape, device=dev, generator=g) * 2 - 1).to(torch.float16)
        y = (x.float() + 0.05 * torch.randn(shape, device=dev, generator=g)).to(torch.float16)
        for temporal in (1, 0):
            To = T - (WIN - 1) * temporal
            win = metrics._gssim_window_on(torch.device(dev), torch.float32 if temporal else torch.float64)
            need = _lib.host("gaussian_ssim_workspace_bytes", C, T, H, W, temporal)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            sums = torch.empty(To, C, dtype=torch.float64, device=dev)
            fn = lambda: _lib.call("gaussian_ssim", x, x.stride(0), x.stride(1), x.stride(2), y, y.stride(0), y.stride(1), y.stride(2),  # noqa: E731
                                   0, C, T, H, W, 1, temporal, win, sums, ws, need)
            ms, lo, hi = timed(fn, a.warmup, a.reps, a.inner)
            positions = C * To * (H - 10) * (W - 10)
            fma = positions * (165 if temporal else 110)
            hbm = 2 * x.numel() * 2 + sums.numel() * 8
            rec = {"case": label, "temporal": temporal, "shape": list(shape), "ms": ms, "ms_min": lo, "ms_max": hi, "positions": positions,
                   "fma": fma, "fp64_TFMAps": fma / ms / 1e9, "hbm_bytes": hbm, "GBps": hbm / ms / 1e6, "workspace_bytes": need,
                   "mean": float(sums.sum().item() / positions)}
            win32 = torch.from_numpy(metrics.gaussian_window(torch.float32 if temporal else torch.float64)).to(dev, torch.float32)
            chunk = 8 if H >= 720 else To
            tfn = lambda: torch_sum(x, y, win32, temporal, chunk)     # noqa: E731
            tms, tlo, thi = timed(tfn, 1, max(2, a.reps // 2), 1)
            rec.update(torch_fp32_ms=tms, torch_fp32_ms_min=tlo, torch_fp32_ms_max=thi,
                       torch_fp32_mean_diff=abs(float(tfn().item()) / positions - rec["mean"]))
            if not a.no_host:
                n = min(To, a.host_frames)
                t0 = time.perf_counter()
                Tn = n + (WIN - 1) * temporal
                qa = metrics_ref.quantise(x[:, :Tn].float().cpu().numpy(), True)
                qb = metrics_ref.quantise(y[:, :Tn].float().cpu().numpy(), True)
                hs = gssim_ref.ssim_map(qa, qb, gssim_ref.window("fp32" if temporal else "fp64"), bool(temporal)).sum(axis=(2, 3)).T
                dt = time.perf_counter() - t0
                rec.update(host_numpy_s=dt * To / n, host_frames_timed=n,
                           host_max_rel_diff=float(np.abs(hs / sums[:n].cpu().numpy() - 1.0).max()))
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del x, y
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
