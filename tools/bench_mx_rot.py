#!/usr/bin/env python3
"""The rotated MXFP4 quantisers (include/hv_mx_rot.h) against the unrotated ones of the same build, on the activation shapes of the
shipped model (M = 119,056 tokens): one process, the kernels alternating inside every repetition, HIP events, warm-up, median.

    python tools/bench_mx_rot.py [--m 119056] [--reps 7] [--out profiles/metrics/bench_mx_rot.json]

Bytes/s are over the bytes a pass has to move: 2 K in, K / 2 + K / 32 out per row.  Inputs are hashed-uniform
(synthetic.hashed_uniform).  The step time of a whole sample_video.py run under --mxfp4-rotate is not measured here."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_gemm_mx4 import BF, rows_of, timed  # noqa: E402
from hunyuanvideo_efficiency_amd import gemm_mx4 as mx, mx_rot, synthetic as syn  # noqa: E402

ROTS = mx_rot.ROTS
KS = [3072, 12288, 15360]


def row_of_times(M, K, ms):
    gbytes = M * (2 * K + K // 2 + K // 32) / 1e9
    row = dict(M=M, K=K, plain_ms=ms[0], plain_tbytes_per_s=gbytes / ms[0])
    for r, t in zip(ROTS, ms[1:]):
        row.update({f"rot{r}_ms": t, f"rot{r}_tbytes_per_s": gbytes / t, f"rot{r}_over_plain_time": t / ms[0]})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=119056)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "bench_mx_rot.json"))
    a = ap.parse_args()
    dev, M = "cuda", a.m
    rows = []
    for K in KS:
        x = rows_of(M, K, f"bench.a{K}", 2.0, dev)
        c, s = mx.quant_rows_mxfp4(x)
        ms = timed([lambda: mx.quant_rows_mxfp4(x, codes=c, scales=s)] +
                   [lambda r=r: mx_rot.quant_rows_mxfp4_rot(x, r, codes=c, scales=s) for r in ROTS], a.reps)
        rows.append(row_of_times(M, K, ms))
        print(json.dumps(rows[-1]), flush=True)
        del x, c, s
        torch.cuda.empty_cache()
    d = 3072
    x = rows_of(M, d, "bench.ln", 2.0, dev)
    sh, sc = (syn.hashed_uniform((d,), "bench.sh", 5) * 0.3).to(BF).to(dev), (syn.hashed_uniform((d,), "bench.sc", 5) * 0.3).to(BF).to(dev)
    c, s = mx.ln_modulate_mxfp4(x, sh, sc)
    ms = timed([lambda: mx.ln_modulate_mxfp4(x, sh, sc, codes=c, scales=s)] +
               [lambda r=r: mx_rot.ln_modulate_mxfp4_rot(x, sh, sc, r, codes=c, scales=s) for r in ROTS], a.reps)
    ln = row_of_times(M, d, ms)
    print(json.dumps(ln), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events, 2 warm-up + %d repetitions, median; kernels alternate inside a "
               "repetition; hashed-uniform inputs; bytes/s over M (2 K + K / 2 + K / 32)" % a.reps, quant_rows=rows, ln_modulate=ln,
               step_time_under_flag="not measured", video_fidelity_under_rotation="not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
