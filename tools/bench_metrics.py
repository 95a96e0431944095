#!/usr/bin/env python3
"""Time the two passes of the reconstruction scoring (csrc/hv_metrics.hip) on one video, default 3 x 129 x 720 x 1280 fp16, with HIP
events: warm-up, then --reps timed repetitions of each pass, median.  In the same process a plain device copy of the same number of
input bytes (both videos) is timed the same way.  Prints one JSON line: bytes read, milliseconds and GB/s of each pass (GB/s =
input bytes / time: what the algorithm must read, not what the halo re-reads), the copy's GB/s (bytes read, as for the passes) and
the ratios.  --host-frame also times tests/metrics_ref.py on one frame of that size on the host (context only).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=4, default=[3, 129, 720, 1280], metavar=("C", "T", "H", "W"))
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--host-frame", action="store_true")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import _lib
    C, T, H, W = a.shape
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    ref = (torch.rand(C, T, H, W, device=dev, generator=g) * 2 - 1).half()
    rec = (ref.float() + 0.05 * torch.randn(C, T, H, W, device=dev, generator=g)).half()
    sse = torch.empty(T, dtype=torch.int64, device=dev)
    minmax = torch.empty(T, 4, dtype=torch.int32, device=dev)
    ssim_sum = torch.empty(T, C, dtype=torch.float64, device=dev)
    ws = torch.empty(_lib.host("video_metrics_workspace_bytes", C, T, H, W), dtype=torch.uint8, device=dev)

    def run(passes):
        _lib.call("video_metrics", ref, ref.stride(0), ref.stride(1), ref.stride(2), rec, rec.stride(0), rec.stride(1), rec.stride(2),
                  0, C, T, H, W, 1, passes, sse, minmax, ssim_sum, ws, ws.numel())

    in_bytes = 2 * ref.numel() * ref.element_size()
    src = torch.cat([ref.reshape(-1), rec.reshape(-1)])
    dst = torch.empty_like(src)
    out = {"shape": [C, T, H, W], "dtype": "fp16", "input_bytes": in_bytes, "warmup": a.warmup, "reps": a.reps}
    for name, fn in (("stats", lambda: run(1)), ("ssim", lambda: run(2)), ("both", lambda: run(3)), ("copy", lambda: dst.copy_(src))):
        med, lo, hi = timed(fn, a.warmup, a.reps)
        out[f"{name}_ms"] = round(med, 4)
        out[f"{name}_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        out[f"{name}_GBps"] = round(in_bytes / med / 1e6, 1)
    out["copy_bytes_moved"] = 2 * in_bytes                   # the copy also writes what it reads
    out["stats_vs_copy"] = round(out["stats_GBps"] / out["copy_GBps"], 3)
    out["ssim_vs_copy"] = round(out["ssim_GBps"] / out["copy_GBps"], 3)
    if a.host_frame:
        import numpy as np
        from tests import metrics_ref
        f1 = metrics_ref.quantise(ref[:, 0].float().cpu().numpy()).transpose(1, 2, 0)
        f2 = metrics_ref.quantise(rec[:, 0].float().cpu().numpy()).transpose(1, 2, 0)
        t0 = time.perf_counter()
        metrics_ref.psnr(f1, f2), metrics_ref.ssim(f1, f2)
        out["host_metrics_ref_one_frame_s"] = round(time.perf_counter() - t0, 4)
        del np
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
