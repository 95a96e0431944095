#!/usr/bin/env python3
"""Time the self-synchronising entropy stage (csrc/hv_mjpeg_sync.hip) against its two yardsticks: the serial stage B of
csrc/hv_mjpeg_read.hip, and Pillow decoding on the host.  The four 129-frame clips of tools/bench_mjpeg_read.py (1280 x 720 and
1920 x 1080, uniform noise and the smooth synthetic clip, quality 90), each in two codings: `pillow` (Pillow's files, no restart markers:
one interval per frame) and `own` (this project's encoder: one interval per MCU row).  Per file, each figure its own entry:

  * `serial_ms`, `sync_ms[sub_bytes]` - stage B alone with everything on the device, HIP events, --warmup + --reps repetitions, the routes
    alternating inside every repetition; median with [min, max].  The results are compared bit for bit.
  * `iters_per_round_mean`, `iters_per_round_max[sub_bytes]` - from the `iters` output: decode iterations of a unit over its rounds.
  * `file_serial_ms`, `file_auto_ms`, `host_ms` - `.avi` in a warm page cache -> the finished tensor through mjpeg_io.read_mjpeg_clip under
    entropy="serial" and entropy="auto" at the default chunk size, and Pillow decoding every frame on the host + upload + value table; wall
    clock around a synchronise, the three routes alternating, --file-reps times each.  `auto_takes` names the stage "auto" chose.

Prints one JSON line per file; --out also writes them to a file (a JSON list).  Needs a GPU."""
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

from tools.bench_mjpeg import make_clip  # noqa: E402

CLIPS = (("720p129f", 1280, 720, 129), ("1080p129f", 1920, 1080, 129))
CONTENTS = ("noise", "smooth")
SUBS = (32, 64, 128, 256, 512)


def timed_alternating(fns, warmup, reps):
    """HIP-event times of every fn, one after the other inside each repetition -> [(median, min, max)]"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--file-reps", type=int, default=3)
    p.add_argument("--frames", type=int, default=None, help="frames per clip (default 129)")
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--only", type=str, default=None, help="run one clip by name")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mjpeg_sync.py needs a GPU: a CPU run can give no time")
    from PIL import Image
    from hunyuanvideo_efficiency_amd import _abi, _lib, mjpeg_io
    from hunyuanvideo_efficiency_amd.dataset import yuv_value_table
    from hunyuanvideo_efficiency_amd.utils.file_utils import frames_uint8
    dev = "cuda:0"
    lanes = _abi.MJPEG_SYNC_MACROS["HV_MJPEG_SYNC_LANES"]
    vtab = yuv_value_table(torch.float16).to(dev)
    lines = []

    def entropy_stage(data, ib, ie, T, H, W, Ri, ipf, huff):
        need = mjpeg_io.coef_bytes(T, H, W)
        want, got = torch.empty(need, dtype=torch.uint8, device=dev), torch.empty(need, dtype=torch.uint8, device=dev)
        status, status2 = torch.empty(T * ipf, dtype=torch.int32, device=dev), torch.empty(T * ipf, dtype=torch.int32, device=dev)
        iters = torch.empty(T * ipf, dtype=torch.int32, device=dev)
        fns = [lambda: _lib.call("mjpeg_decode_coefs", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, want, need, status)]
        for sub in SUBS:
            fns.append(lambda sub=sub: _lib.call("mjpeg_decode_coefs_sync", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, sub, got, need, status2, None))
        times = timed_alternating(fns, a.warmup, a.reps)
        assert not bool(status.any()), "the bench stream does not decode"
        rec = {"serial_ms": round(times[0][0], 3), "serial_ms_min_max": [round(times[0][1], 3), round(times[0][2], 3)], "sync_ms": {},
               "sync_ms_min_max": {}, "iters_per_round_mean": {}, "iters_per_round_max": {}, "sync_equals_serial": True}
        lens = (ie - ib).clamp(min=0)
        for sub, t in zip(SUBS, times[1:]):
            got.zero_()
            _lib.call("mjpeg_decode_coefs_sync", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, sub, got, need, status2, iters)
            rec["sync_equals_serial"] = rec["sync_equals_serial"] and torch.equal(got, want) and torch.equal(status, status2) and bool((iters > 0).all())
            rounds = ((lens + sub - 1) // sub + lanes - 1) // lanes
            per_round = iters.double() / rounds.clamp(min=1).double()
            rec["sync_ms"][str(sub)] = round(t[0], 3)
            rec["sync_ms_min_max"][str(sub)] = [round(t[1], 3), round(t[2], 3)]
            rec["iters_per_round_mean"][str(sub)] = round(float(iters.sum()) / float(rounds.sum()), 2)
            rec["iters_per_round_max"][str(sub)] = round(float(per_round.max()), 2)
        return rec

    def file_routes(path):
        ref, _ = mjpeg_io.read_mjpeg_clip(path, dev, entropy="serial")                  # warm: pinned allocations, page cache
        mjpeg_io.read_mjpeg_clip(path, dev, entropy="auto")
        s = {"file_serial_ms": [], "file_auto_ms": [], "host_ms": []}
        equal = True
        for _ in range(a.file_reps):
            for key, entropy in (("file_serial_ms", "serial"), ("file_auto_ms", "auto")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                clip, _ = mjpeg_io.read_mjpeg_clip(path, dev, entropy=entropy)
                torch.cuda.synchronize()
                s[key].append(time.perf_counter() - t0)
                equal = equal and torch.equal(clip, ref)
                del clip
            t0 = time.perf_counter()
            raw = open(path, "rb").read()
            frames = [np.asarray(Image.open(io.BytesIO(raw[o:o + n])).convert("RGB")) for o, n in mjpeg_io.parse_avi(path)[3]]
            host = vtab[torch.from_numpy(np.stack(frames)).to(dev).long()].permute(3, 0, 1, 2).contiguous()
            torch.cuda.synchronize()
            s["host_ms"].append(time.perf_counter() - t0)
            equal = equal and torch.equal(host, ref)
            del host, frames, raw
        rec = {"routes_equal": equal}
        for key, v in s.items():
            rec[key] = round(statistics.median(v) * 1e3, 2)
            rec[key + "_all"] = [round(t * 1e3, 2) for t in v]
        rec["host_over_auto"] = round(rec["host_ms"] / rec["file_auto_ms"], 2)
        rec["serial_over_auto"] = round(rec["file_serial_ms"] / rec["file_auto_ms"], 2)
        return rec

    with tempfile.TemporaryDirectory() as tmp:
        for name, W, H, T in CLIPS:
            if a.only and a.only != name:
                continue
            T = a.frames or T
            for content in CONTENTS:
                x = make_clip(content, torch.float16, W, H, T, True, dev)
                for coding in ("pillow", "own"):
                    path = os.path.join(tmp, f"{name}_{content}_{coding}.avi")
                    base = {"case": f"{name}_{content}_{coding}", "size": [W, H], "frames": T, "content": content, "coding": coding,
                            "quality": a.quality, "warmup": a.warmup, "reps": a.reps, "file_reps": a.file_reps,
                            "device": torch.cuda.get_device_name(0), "sub_bytes_default": mjpeg_io.SYNC_SUB_BYTES,
                            "sync_min_interval_bytes": mjpeg_io.SYNC_MIN_INTERVAL_BYTES}
                    if coding == "own":
                        scan, offsets, rows = mjpeg_io._clip_to_intervals(x, a.quality, True, "bench")
                        Ri, ipf = (W + 15) // 16, rows
                        ib, ie = offsets[:-1].contiguous(), offsets[1:].contiguous()
                        huff = mjpeg_io.huff_list(mjpeg_io._ANNEX_K_HUFF)
                        data, scan_bytes = scan, scan.numel()
                        mjpeg_io.write_mjpeg_clip(x, path, 24, a.quality, True)
                    else:
                        jpegs = []
                        for frame in frames_uint8(x[None].cpu().float(), True):
                            b = io.BytesIO()
                            Image.fromarray(frame).save(b, "JPEG", quality=a.quality, subsampling=2)
                            jpegs.append(b.getvalue())
                        open(path, "wb").write(mjpeg_io.avi_file(jpegs, W, H, 24))
                        parsed, pos = [], 0
                        for j in jpegs:
                            fr = mjpeg_io.parse_jpeg(j)
                            parsed.append(fr._replace(scan_begin=fr.scan_begin + pos, scan_end=fr.scan_end + pos))
                            pos += len(j)
                        assert all(f[:5] == parsed[0][:5] for f in parsed) and parsed[0].Ri == 0
                        data = torch.frombuffer(bytearray(b"".join(jpegs)), dtype=torch.uint8).to(dev)
                        ib = torch.tensor([f.scan_begin for f in parsed], dtype=torch.int64, device=dev)
                        ie = torch.tensor([f.scan_end for f in parsed], dtype=torch.int64, device=dev)
                        Ri, ipf, huff = 0, 1, mjpeg_io.huff_list(parsed[0].huff)
                        scan_bytes = int((ie - ib).sum())
                        del jpegs
                    print(f"# {base['case']}: coded, {scan_bytes} scan bytes", flush=True)
                    rec = dict(base, scan_bytes=scan_bytes, intervals=T * ipf, mean_interval_bytes=round(scan_bytes / (T * ipf), 1),
                               auto_takes="sync" if mjpeg_io.use_sync("auto", scan_bytes, T * ipf) else "serial", file_bytes=os.path.getsize(path))
                    rec.update(entropy_stage(data, ib, ie, T, H, W, Ri, ipf, huff))
                    print(f"# {base['case']}: entropy stage timed", flush=True)
                    del data, ib, ie
                    rec.update(file_routes(path))
                    os.remove(path)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "w") as f:
                            json.dump(lines, f, indent=1)
                            f.write("\n")
                del x
                torch.cuda.empty_cache()
    return lines


if __name__ == "__main__":
    main()
