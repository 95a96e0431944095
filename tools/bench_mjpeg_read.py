#!/usr/bin/env python3
"""Time the Motion-JPEG reader (csrc/hv_mjpeg_read.hip) and the whole file-to-tensor path.  129 frames at 1280 x 720 and at 1920 x 1080,
each on uniform noise (the densest stream a decoder can meet) and on the smooth synthetic clip of tools/bench_mjpeg.py, coded at quality
90 by this project's encoder (one restart interval per MCU row) and decoded to fp16.  Per case, each figure its own entry:

  * `find_restarts_ms`, `decode_coefs_ms`, `coefs_to_clip_ms` - the three stages alone with everything on the device (HIP events: warm-up,
    then --reps repetitions, median, with min and max).  Stage B also as `decode_input_GBps` (entropy-coded bytes over its time), with
    `decoders` (restart intervals = serial decoders) and `decoders_per_cu`.  Stage C also as `clip_GBps` over `clip_bytes` = the workspace
    read plus the clip written, and `clip_of_stream_copy` against the 6.3 TB/s streaming-copy figure the YUV kernels are compared with.
  * `file_ms`    - mjpeg_io.read_mjpeg_clip from the `.avi` in a warm page cache to the finished tensor (wall clock around a synchronise):
    container and header parsing, pinned staging, upload, the three stages, one status read-back behind the last chunk.
  * `host_ms`    - the route it replaces, in the same call, alternating, --file-reps times each: Pillow decoding every frame of the same
    file, torch.from_numpy, upload, the value table.  `host_over_file` is the ratio of the medians.
  * `foreign_*`  - the same clip coded by Pillow WITHOUT restart markers (one interval per frame: `foreign_decoders` = the frame count), the
    stated worst case of a serial Huffman lane: `foreign_decode_coefs_ms`, `foreign_file_ms`, `foreign_file_bytes`.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402
from tools.bench_mjpeg import make_clip  # noqa: E402

CLIPS = (("720p129f", 1280, 720, 129), ("1080p129f", 1920, 1080, 129))
CONTENTS = ("noise", "smooth")
STREAM_COPY_TBPS = 6.3


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--file-reps", type=int, default=3)
    p.add_argument("--frames", type=int, default=None, help="frames per clip (default 129)")
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--only", type=str, default=None, help="run one clip by name")
    p.add_argument("--no-foreign", action="store_true", help="skip the Pillow-coded file without restart markers")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mjpeg_read.py needs a GPU: a CPU run can give no time")
    from PIL import Image
    from hunyuanvideo_efficiency_amd import _lib, mjpeg_io
    from hunyuanvideo_efficiency_amd.dataset import yuv_value_table
    from hunyuanvideo_efficiency_amd.utils.file_utils import frames_uint8
    dev = "cuda:0"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    vtab = yuv_value_table(torch.float16).to(dev)
    lines = []

    def stage_b_c(data, ib, ie, T, H, W, Ri, ipf, huff, quant, out):
        need = mjpeg_io.coef_bytes(T, H, W)
        coefs = torch.empty(need, dtype=torch.uint8, device=dev)
        status = torch.empty(T * ipf, dtype=torch.int32, device=dev)
        b = timed(lambda: _lib.call("mjpeg_decode_coefs", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, coefs, need, status), a.warmup, a.reps)
        assert not bool(status.any()), "the bench stream does not decode"
        c = timed(lambda: _lib.call("mjpeg_coefs_to_clip", coefs, need, quant, vtab, out, 0, out.stride(0), out.stride(1), out.stride(2), T, H, W),
                  a.warmup, a.reps)
        return b, c, need

    with tempfile.TemporaryDirectory() as tmp:
        for name, W, H, T in CLIPS:
            if a.only and a.only != name:
                continue
            T = a.frames or T
            for content in CONTENTS:
                x = make_clip(content, torch.float16, W, H, T, True, dev)
                scan, offsets, rows = mjpeg_io._clip_to_intervals(x, a.quality, True, "bench")
                mcus, ipf = (W + 15) // 16, rows
                huff = mjpeg_io.huff_list(mjpeg_io._ANNEX_K_HUFF)
                q = mjpeg_io.quant_tables(a.quality)
                out = torch.empty(3, T, H, W, dtype=torch.float16, device=dev)
                sb, se = offsets[:-1:rows].contiguous(), offsets[rows::rows].contiguous()
                ib, ie = torch.empty(T * ipf, dtype=torch.int64, device=dev), torch.empty(T * ipf, dtype=torch.int64, device=dev)
                found = torch.empty(T, dtype=torch.int32, device=dev)
                a_ms = timed(lambda: _lib.call("mjpeg_find_restarts", scan, scan.numel(), sb, se, T, ipf, ib, ie, found), a.warmup, a.reps)
                assert found.tolist() == [ipf - 1] * T
                b_ms, c_ms, need = stage_b_c(scan, ib, ie, T, H, W, mcus, ipf, huff, q[0] + q[1], out)
                clip_bytes = need + out.numel() * out.element_size()
                rec = {"case": f"{name}_{content}", "size": [W, H], "frames": T, "content": content, "quality": a.quality, "dtype": "float16",
                       "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0), "compute_units": cus,
                       "scan_bytes": scan.numel(),
                       "find_restarts_ms": round(a_ms[0], 4), "find_restarts_ms_min_max": [round(a_ms[1], 4), round(a_ms[2], 4)],
                       "decode_coefs_ms": round(b_ms[0], 4), "decode_coefs_ms_min_max": [round(b_ms[1], 4), round(b_ms[2], 4)],
                       "decode_input_GBps": round(scan.numel() / b_ms[0] / 1e6, 2), "decoders": T * ipf, "decoders_per_cu": round(T * ipf / cus, 1),
                       "coefs_to_clip_ms": round(c_ms[0], 4), "coefs_to_clip_ms_min_max": [round(c_ms[1], 4), round(c_ms[2], 4)],
                       "workspace_bytes": need, "clip_bytes": clip_bytes, "clip_GBps": round(clip_bytes / c_ms[0] / 1e6, 1),
                       "clip_of_stream_copy": round(clip_bytes / c_ms[0] / 1e6 / (STREAM_COPY_TBPS * 1e3), 3),
                       "encoder_kernel_ms_720p": [1.2, 1.4]}
                del scan, offsets, ib, ie
                path = os.path.join(tmp, f"{name}_{content}.avi")
                mjpeg_io.write_mjpeg_clip(x, path, 24, a.quality, True)
                ref, _ = mjpeg_io.read_mjpeg_clip(path, dev)                          # warm: pinned allocations, page cache
                file_s, host_s, equal = [], [], True
                for _ in range(a.file_reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    clip, _ = mjpeg_io.read_mjpeg_clip(path, dev)
                    torch.cuda.synchronize()
                    file_s.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    raw = open(path, "rb").read()
                    frames = [np.asarray(Image.open(io.BytesIO(raw[o:o + n])).convert("RGB")) for o, n in mjpeg_io.parse_avi(path)[3]]
                    host = vtab[torch.from_numpy(np.stack(frames)).to(dev).long()].permute(3, 0, 1, 2).contiguous()
                    torch.cuda.synchronize()
                    host_s.append(time.perf_counter() - t0)
                    equal = equal and torch.equal(clip, ref) and torch.equal(host, clip)
                    del host, frames, raw, clip
                rec.update(file_bytes=os.path.getsize(path), file_ms=round(statistics.median(file_s) * 1e3, 2),
                           file_ms_all=[round(t * 1e3, 2) for t in file_s], host_ms=round(statistics.median(host_s) * 1e3, 2),
                           host_ms_all=[round(t * 1e3, 2) for t in host_s],
                           host_over_file=round(statistics.median(host_s) / statistics.median(file_s), 2), host_equals_gpu=equal)
                os.remove(path)
                del ref
                if not a.no_foreign:
                    jpegs = []
                    for frame in frames_uint8(x[None].cpu().float(), True):
                        b = io.BytesIO()
                        Image.fromarray(frame).save(b, "JPEG", quality=a.quality, subsampling=2)
                        jpegs.append(b.getvalue())
                    open(path, "wb").write(mjpeg_io.avi_file(jpegs, W, H, 24))
                    blob, parsed, pos = b"".join(jpegs), [], 0
                    for j in jpegs:
                        fr = mjpeg_io.parse_jpeg(j)
                        parsed.append(fr._replace(scan_begin=fr.scan_begin + pos, scan_end=fr.scan_end + pos))
                        pos += len(j)
                    assert all(f[:5] == parsed[0][:5] for f in parsed) and parsed[0].Ri == 0
                    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
                    fb = torch.tensor([f.scan_begin for f in parsed], dtype=torch.int64, device=dev)
                    fe = torch.tensor([f.scan_end for f in parsed], dtype=torch.int64, device=dev)
                    fb_ms, _, _ = stage_b_c(data, fb, fe, T, H, W, 0, 1, mjpeg_io.huff_list(parsed[0].huff),
                                            list(parsed[0].quant[0]) + list(parsed[0].quant[1]), out)
                    mjpeg_io.read_mjpeg_clip(path, dev)
                    f_s = []
                    for _ in range(a.file_reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        mjpeg_io.read_mjpeg_clip(path, dev)
                        torch.cuda.synchronize()
                        f_s.append(time.perf_counter() - t0)
                    rec.update(foreign_decoders=T, foreign_scan_bytes=int((fe - fb).sum()), foreign_file_bytes=os.path.getsize(path),
                               foreign_decode_coefs_ms=round(fb_ms[0], 3), foreign_decode_coefs_ms_min_max=[round(fb_ms[1], 3), round(fb_ms[2], 3)],
                               foreign_decode_input_GBps=round(int((fe - fb).sum()) / fb_ms[0] / 1e6, 3),
                               foreign_file_ms=round(statistics.median(f_s) * 1e3, 2), foreign_file_ms_all=[round(t * 1e3, 2) for t in f_s])
                    os.remove(path)
                    del data, jpegs, blob
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del x, out
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
