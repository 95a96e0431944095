#!/usr/bin/env python3
"""Time the Motion-JPEG kernels (csrc/hv_mjpeg.hip) and the whole tensor-to-file path.  Two clips, a 129-frame 1280 x 720 fp32 clip in
[0, 1] (what the pipeline returns) and a 129-frame 1920 x 1080 fp16 clip in [-1, 1] (a VAE reconstruction), each on two contents: uniform
noise (the densest stream a coder can meet) and a smooth synthetic clip (drifting sinusoids, closer to what a video holds), at the default
quality.  Per case:

  * `measure_ms`, `write_ms` - hv_mjpeg_measure and hv_mjpeg_write alone with everything on the device (HIP events: warm-up, then --reps
    repetitions, median, with min and max); `scan_bytes` what the second writes; `input_GBps` the input bytes over each time (both
    kernels read the whole clip).
  * `clip_to_jpeg_ms` - mjpeg_io.clip_to_jpeg: both kernels, the prefix sum and the one synchronisation that sizes the output (wall clock).
  * `file_ms`    - mjpeg_io.write_mjpeg_clip from the device tensor to the finished `.avi` on local disk (wall clock around a
    synchronise): kernels, copy through pinned staging, file writes.  `file_bytes` next to `y4m_bytes`, the size of the `.y4m` of the same
    clip (header + frames of W * H * 3 / 2 + 6 bytes), and their ratio.
  * `host_ms`    - the route it replaces, for the same tensor: `.cpu().float()`, utils/file_utils.py:frames_uint8 and Pillow's JPEG
    encoder per frame at the same quality, 4:2:0, into memory (wall clock; no container write).  `host_jpeg_bytes` is what it produces.
    The two routes alternate, --file-reps times each; `host_over_file` is the ratio of the medians.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402

CLIPS = (("fp32_720p129f", torch.float32, 1280, 720, 129, False), ("fp16_1080p129f", torch.float16, 1920, 1080, 129, True))
CONTENTS = ("noise", "smooth")


def make_clip(content, dtype, W, H, T, rescale, dev):
    if content == "noise":
        x = torch.rand(3, T, H, W, generator=torch.Generator(device=dev).manual_seed(0), device=dev, dtype=torch.float32)
    else:
        t = torch.arange(T, device=dev, dtype=torch.float32)[:, None, None]
        y = torch.arange(H, device=dev, dtype=torch.float32)[None, :, None]
        c = torch.arange(W, device=dev, dtype=torch.float32)[None, None, :]
        x = torch.stack([(torch.sin((c + 7 * t) / 40) + 1) / 2 * torch.ones_like(y), (torch.cos(y / 30 + t / 9) + 1) / 2 * torch.ones_like(c),
                         ((c + y + 5 * t) % 256) / 255])
    return (x * 2 - 1 if rescale else x).to(dtype)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--file-reps", type=int, default=3)
    p.add_argument("--frames", type=int, default=None, help="frames per clip (default 129)")
    p.add_argument("--quality", type=int, default=None)
    p.add_argument("--only", type=str, default=None, help="run one clip by name")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mjpeg.py needs a GPU: a CPU run can give no time")
    from PIL import Image
    from hunyuanvideo_efficiency_amd import _lib, mjpeg_io
    from hunyuanvideo_efficiency_amd.utils.file_utils import frames_uint8
    from hunyuanvideo_efficiency_amd.video_io import y4m_header
    dev = "cuda:0"
    quality = mjpeg_io.DEFAULT_QUALITY if a.quality is None else a.quality
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, dtype, W, H, T, rescale in CLIPS:
            if a.only and a.only != name:
                continue
            T = a.frames or T
            for content in CONTENTS:
                x = make_clip(content, dtype, W, H, T, rescale, dev)
                rows = (H + mjpeg_io.MCU - 1) // mjpeg_io.MCU
                args = (x, 0 if dtype == torch.float16 else 1, 3, x.stride(0), x.stride(1), x.stride(2), T, H, W, int(rescale), quality)
                sizes = torch.empty(T * rows, dtype=torch.int32, device=dev)
                m_med, m_lo, m_hi = timed(lambda: _lib.call("mjpeg_measure", *args, sizes), a.warmup, a.reps)
                offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), sizes.to(torch.int64).cumsum(0)])
                scan = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=dev)
                w_med, w_lo, w_hi = timed(lambda: _lib.call("mjpeg_write", *args, offsets, scan), a.warmup, a.reps)
                in_bytes = x.numel() * x.element_size()
                rec = {"case": f"{name}_{content}", "dtype": str(dtype).replace("torch.", ""), "size": [W, H], "frames": T, "content": content,
                       "quality": quality, "warmup": a.warmup, "reps": a.reps,
                       "measure_ms": round(m_med, 4), "measure_ms_min_max": [round(m_lo, 4), round(m_hi, 4)],
                       "write_ms": round(w_med, 4), "write_ms_min_max": [round(w_lo, 4), round(w_hi, 4)],
                       "input_bytes": in_bytes, "scan_bytes": scan.numel(), "bytes_per_pixel": round(scan.numel() / (T * W * H), 4),
                       "input_GBps": [round(in_bytes / m_med / 1e6, 1), round(in_bytes / w_med / 1e6, 1)],
                       "device": torch.cuda.get_device_name(0)}
                del scan, offsets
                path = os.path.join(tmp, f"{name}_{content}.avi")
                mjpeg_io.write_mjpeg_clip(x, path, 24, quality, rescale)             # warm: pinned allocations, page cache
                jpeg_s, file_s, host_s, host_bytes = [], [], [], 0
                for _ in range(a.file_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = mjpeg_io.clip_to_jpeg(x, quality, rescale)
                    torch.cuda.synchronize()
                    jpeg_s.append(time.perf_counter() - t0)
                    del out
                    t0 = time.perf_counter()
                    mjpeg_io.write_mjpeg_clip(x, path, 24, quality, rescale)
                    torch.cuda.synchronize()
                    file_s.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    host = x[None].cpu().float()
                    host_bytes = 0
                    for frame in frames_uint8(host, rescale):
                        b = io.BytesIO()
                        Image.fromarray(frame).save(b, "JPEG", quality=quality, subsampling=2)
                        host_bytes += b.tell()
                    host_s.append(time.perf_counter() - t0)
                    del host
                y4m = len(y4m_header(W, H, 24)) + T * (6 + W * H * 3 // 2)
                rec.update(clip_to_jpeg_ms=round(statistics.median(jpeg_s) * 1e3, 2), file_ms=round(statistics.median(file_s) * 1e3, 2),
                           file_ms_all=[round(t * 1e3, 2) for t in file_s], file_bytes=os.path.getsize(path), y4m_bytes=y4m,
                           y4m_over_file=round(y4m / os.path.getsize(path), 2), host_ms=round(statistics.median(host_s) * 1e3, 2),
                           host_ms_all=[round(t * 1e3, 2) for t in host_s], host_jpeg_bytes=host_bytes,
                           host_over_file=round(statistics.median(host_s) / statistics.median(file_s), 2))
                os.remove(path)
                print(json.dumps(rec), flush=True)
                lines.append(rec)
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
