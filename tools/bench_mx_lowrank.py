#!/usr/bin/env python3
"""The MXFP4 GEMM with a low-rank bf16 branch and its quantise + down-project pass (include/hv_mx_lowrank.h) against the branch-less
kernels of the same build, on the linear shapes of the shipped model (M = 119,056 tokens): one process, the kernels alternating inside
every repetition, HIP events, warm-up, median.

    python tools/bench_mx_lowrank.py [--m 119056] [--reps 7] [--out profiles/metrics/bench_mx_lowrank.json]

Ratios are times over the branch-less kernel's time.  Inputs are hashed-uniform (synthetic.hashed_uniform).  The step time of a whole
sample_video.py run under --mxfp4-lowrank and video fidelity are not measured here."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_gemm_mx4 import BF, SHAPES, rows_of, timed  # noqa: E402
from hunyuanvideo_efficiency_amd import gemm_mx4 as mx, mx_lowrank as lr, ops, synthetic as syn  # noqa: E402

RANKS = (32, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=119056)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "bench_mx_lowrank.json"))
    a = ap.parse_args()
    dev, M = "cuda", a.m
    gemms, quants = [], []
    for N, K in SHAPES:
        x, w = rows_of(M, K, f"bench.a{K}", 2.0, dev), rows_of(N, K, f"bench.w{N}.{K}", 1.0, dev)
        dn, up = rows_of(128, K, f"bench.dn{K}", 0.05, dev), rows_of(N, 128, f"bench.up{N}", 1.0, dev)
        a4, a4s, t = lr.quant_rows_mxfp4_lr(x, dn)
        w4, w4s = mx.quant_rows_mxfp4(w)
        out = torch.empty(M, N, dtype=BF, device=dev)
        ms = timed([lambda: mx.gemm_mxfp4(a4, a4s, w4, w4s, out=out)] +
                   [lambda r=r: lr.gemm_mxfp4_lr(a4, a4s, w4, w4s, t[:, :r], up[:, :r], out=out) for r in RANKS], a.reps)
        gemms.append(dict(M=M, N=N, K=K, plain_ms=ms[0], **{f"r{r}_ms": v for r, v in zip(RANKS, ms[1:])},
                          **{f"r{r}_over_plain_time": v / ms[0] for r, v in zip(RANKS, ms[1:])}))
        print(json.dumps(gemms[-1]), flush=True)
        if K not in [q["K"] for q in quants]:
            ms = timed([lambda: mx.quant_rows_mxfp4(x, codes=a4, scales=a4s)] +
                       [lambda r=r: lr.quant_rows_mxfp4_lr(x, dn[:r], codes=a4, scales=a4s, t=t[:, :r]) for r in RANKS], a.reps)
            quants.append(dict(M=M, K=K, plain_ms=ms[0], **{f"r{r}_ms": v for r, v in zip(RANKS, ms[1:])},
                               **{f"r{r}_over_plain_time": v / ms[0] for r, v in zip(RANKS, ms[1:])}))
            print(json.dumps(quants[-1]), flush=True)
        del x, w, dn, up, a4, a4s, t, w4, w4s, out
        torch.cuda.empty_cache()
    d = 3072
    x, dn = rows_of(M, d, "bench.ln", 2.0, dev), rows_of(128, d, "bench.dnln", 0.05, dev)
    sh, sc = (syn.hashed_uniform((d,), "bench.sh", 5) * 0.3).to(BF).to(dev), (syn.hashed_uniform((d,), "bench.sc", 5) * 0.3).to(BF).to(dev)
    c, s = mx.ln_modulate_mxfp4(x, sh, sc)
    xm, t = torch.empty_like(x), torch.empty(M, 128, dtype=BF, device=dev)

    def two_pass(r):
        ops.ln_modulate(x, sh, sc, out=xm)
        lr.quant_rows_mxfp4_lr(xm, dn[:r], codes=c, scales=s, t=t[:, :r])

    ms = timed([lambda: mx.ln_modulate_mxfp4(x, sh, sc, codes=c, scales=s)] + [lambda r=r: two_pass(r) for r in RANKS], a.reps)
    ln = dict(M=M, D=d, fused_ln_mxfp4_ms=ms[0], **{f"ln_then_lr{r}_ms": v for r, v in zip(RANKS, ms[1:])},
              **{f"ln_then_lr{r}_over_fused_time": v / ms[0] for r, v in zip(RANKS, ms[1:])})
    print(json.dumps(ln), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events, 2 warm-up + %d repetitions, median; kernels alternate inside a "
               "repetition; hashed-uniform inputs; ratios are times over the branch-less kernel of the same build and process" % a.reps,
               gemm=gemms, quant_rows=quants, ln_modulate=ln, step_time_under_flag="not measured", video_fidelity="not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
