#!/usr/bin/env python3
"""Time the temporal-spectrum kernel (csrc/hv_spectrum.hip) with HIP events: warm-up, then --reps timed repetitions, median.  Three
cases: gray mode on a 3 x 129 x 720 x 1280 fp16 clip, raw mode on a 16 x 33 x 90 x 160 fp32 latent, gray mode on a 600-frame
3 x 270 x 480 fp16 clip.  Beside each device time:

  * `host_fft_s` - the reference's way (theory_analysis.ipynb cell 2) on this machine's CPU: the device-to-host copy of the tensor the
    device path never makes, then np.abs(np.fft.fft(signal, axis=0)).mean(axis=1) on the [T, series] signal (the gray bytes are
    formed on the device beforehand, untimed: the reference gets them from a video decoder).  One repetition; --no-host skips it.
  * `hbm_bytes` - what the algorithm must read: the tensor once plus the twiddle table (the table and the re-read of the series by the
    column tiles of one row tile are cache traffic, not counted) - and `mfma_flops` = 2 x padded series x padded frames x table columns,
    the fp32-MFMA work the launch issues, with the time each would take alone at 8 TB/s and 157.3 TF/s: which side the launch sits on.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402

FP32_ROOF_TF = 157.3            # MI355X fp32-input MFMA peak
HBM_ROOF_TBPS = 8.0             # MI355X HBM3E peak

CASES = (("gray_720p129f", "gray", (3, 129, 720, 1280), torch.float16),
         ("raw_latent_33f", "raw", (16, 33, 90, 160), torch.float32),
         ("gray_270p600f", "gray", (3, 600, 270, 480), torch.float16))


def launch_counts(mode, shape, elem):
    """(algorithmic HBM bytes, fp32-MFMA flops) of one launch, from the shapes and the kernel's tile sizes (256 series x 64 columns x 32
    frames)"""
    C, T, H, W = shape
    n = (H * W) if mode == "gray" else C * H * W
    tpad = -(-T // 32) * 32
    cols = max(1, -(-(T // 2) // 32)) * 64
    return C * T * H * W * elem + tpad * cols * 4 + 2 * (T // 2 + 1) * 8, 2 * (-(-n // 256) * 256) * tpad * cols


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--no-host", action="store_true", help="skip the host FFT")
    p.add_argument("--only", type=str, default=None, help="run one case by name")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectrum.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import metrics
    dev = "cuda:0"
    lines = []
    for name, mode, shape, dtype in CASES:
        if a.only and a.only != name:
            continue
        C, T, H, W = shape
        g = torch.Generator(device=dev).manual_seed(0)
        # a drifting picture plus noise: values in [-1, 1] for the clips, latent-like for the raw case
        x = torch.rand(C, 1, H, W, device=dev, generator=g) * 1.2 - 0.6
        x = x + 0.3 * torch.sin(torch.linspace(0, 9.0, T, device=dev)).view(1, T, 1, 1) + 0.1 * torch.randn(C, T, H, W, device=dev, generator=g)
        x = (x.clamp(-1, 1) if mode == "gray" else 3.0 * x).to(dtype)
        metrics.spectrum_sums(x, mode)                          # builds and caches the twiddle table
        med, lo, hi = timed(lambda: metrics.spectrum_sums(x, mode), a.warmup, a.reps)
        hbm, flops = launch_counts(mode, shape, x.element_size())
        out = {"case": name, "mode": mode, "shape": list(shape), "dtype": str(dtype).split(".")[-1], "warmup": a.warmup, "reps": a.reps,
               "ms": round(med, 4), "ms_min_max": [round(lo, 4), round(hi, 4)], "hbm_bytes": hbm, "mfma_flops": flops,
               "GBps": round(hbm / med / 1e6, 1), "mfma_TFps": round(flops / med / 1e9, 2),
               "ms_at_hbm_roof": round(hbm / (HBM_ROOF_TBPS * 1e9), 4), "ms_at_fp32_mfma_roof": round(flops / (FP32_ROOF_TF * 1e9), 4)}
        out["bound_side"] = "mfma" if out["ms_at_fp32_mfma_roof"] > out["ms_at_hbm_roof"] else "hbm"
        if not a.no_host:
            if mode == "gray":
                wr, wg, wb, rnd, shift = metrics.GRAY_LUMA
                q = (((x.float() + 1.0) / 2.0).clamp(0, 1) * 255).to(torch.uint8).to(torch.int32)
                sig_dev = ((wr * q[0] + wg * q[1] + wb * q[2] + rnd) >> shift).to(torch.uint8).reshape(T, -1)
            else:
                sig_dev = x.permute(1, 0, 2, 3).reshape(T, -1).contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x.cpu()                                             # the copy the device path avoids
            t1 = time.perf_counter()
            sig = sig_dev.cpu().numpy()                         # untimed stand-in for the decoder's gray frames
            t2 = time.perf_counter()
            host = np.abs(np.fft.fft(sig, axis=0)).mean(axis=1)
            t3 = time.perf_counter()
            out["d2h_s"], out["host_fft_s"] = round(t1 - t0, 4), round((t1 - t0) + (t3 - t2), 4)
            m = metrics.temporal_spectrum(x, mode)
            out["max_rel_diff_vs_host_fft"] = float(np.max(np.abs(m["magnitude"] - host) / np.maximum(host, 1e-30)))
            out["host_over_device"] = round(out["host_fft_s"] * 1e3 / med, 1)
            del sig, host, sig_dev
        print(json.dumps(out), flush=True)
        lines.append(out)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
