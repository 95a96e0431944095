#!/usr/bin/env python3
"""Time the raw YUV 4:2:0 -> clip kernel (csrc/hv_yuv.hip) and the whole file-to-tensor path.  Three cases on a 129-frame 1920 x 1080
clip of random bytes, fp16 output: I420 at source size, the same clip to 240 rows (426 x 240), the same clip as NV12.  Per case:

  * `kernel_ms`  - hv_yuv420_to_clip alone with everything on the device (HIP events: warm-up, then --reps repetitions, median);
    `bytes` = source bytes read + output bytes written (for the resized case: the whole source, although taps of a strong downscale
    skip most of it), `GBps` the resulting rate, next to `copy_GBps_ref` = 6300, the achievable streaming-copy rate of the MI355X's
    HBM: what a kernel that only moved these bytes would reach.
  * `file_ms`    - dataset.read_yuv_clip from a file on local disk to the finished tensor (wall clock, page cache warm after the first
    repetition): read, pinned staging, upload, kernel.  The read and the upload dominate it; `file_GBps` is file bytes per second.
  * `host_s`     - the numpy restatement (tests/yuv_ref.py) of the same conversion on this machine's CPU, one repetition on
    --host-frames frames scaled to the clip's length; --no-host skips it.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402

COPY_GBPS = 6300.0              # MI355X HBM3E: achievable streaming rate (8 TB/s peak)
W, H, T = 1920, 1080, 129
CASES = (("i420_1080p129f", "I420", None), ("i420_1080p129f_to_240", "I420", 240), ("nv12_1080p129f", "NV12", None))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--file-reps", type=int, default=3)
    p.add_argument("--host-frames", type=int, default=4, help="frames the numpy restatement converts (its time is scaled to the clip)")
    p.add_argument("--no-host", action="store_true")
    p.add_argument("--only", type=str, default=None, help="run one case by name")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import dataset
    dev = "cuda:0"
    frame = W * H * 3 // 2
    host = np.random.default_rng(0).integers(0, 256, size=(T, frame), dtype=np.uint8)
    raw = torch.from_numpy(host.reshape(-1)).to(dev)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, f"bench_30fps_{W}x{H}.yuv")
        host.tofile(path)
        for name, fmt, th in CASES:
            if a.only and a.only != name:
                continue
            size = None if th is None else dataset.target_size(W, H, th)
            OW, OH = (W, H) if size is None else size
            out = torch.empty(3, T, OH, OW, dtype=torch.float16, device=dev)
            dataset.yuv_to_clip(raw, W, H, fmt, size=size, out=out)              # builds and caches the tables
            med, lo, hi = timed(lambda: dataset.yuv_to_clip(raw, W, H, fmt, size=size, out=out), a.warmup, a.reps)
            nbytes = raw.numel() + out.numel() * out.element_size()
            rec = {"case": name, "format": fmt, "source": [W, H], "frames": T, "output": [OW, OH], "dtype": "float16", "warmup": a.warmup,
                   "reps": a.reps, "kernel_ms": round(med, 4), "kernel_ms_min_max": [round(lo, 4), round(hi, 4)], "bytes": nbytes,
                   "GBps": round(nbytes / med / 1e6, 1), "copy_GBps_ref": COPY_GBPS, "share_of_copy_rate": round(nbytes / med / 1e6 / COPY_GBPS, 3)}
            del out
            times = []
            for _ in range(a.file_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clip, _ = dataset.read_yuv_clip(path, dev, fmt, target_height=th)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                del clip
            rec["file_ms"] = round(sorted(times)[len(times) // 2] * 1e3, 2)
            rec["file_ms_all"] = [round(t * 1e3, 2) for t in times]
            rec["file_GBps"] = round(raw.numel() / (rec["file_ms"] * 1e-3) / 1e9, 2)
            if not a.no_host:
                from tests import yuv_ref
                n = min(a.host_frames, T)
                t0 = time.perf_counter()
                ref = yuv_ref.clip(host[:n], W, H, fmt, torch.float16, size)
                rec["host_s"] = round((time.perf_counter() - t0) * T / n, 2)
                rec["host_frames_timed"] = n
                got = dataset.yuv_to_clip(raw[:n * frame], W, H, fmt, size=size)
                rec["equal_to_host"] = bool(torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16)))
                rec["host_over_kernel"] = round(rec["host_s"] * 1e3 / med, 1)
                del ref, got
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
