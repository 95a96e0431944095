#!/usr/bin/env python3
"""MXFP6 linears against the bf16, FP8 and MXFP4 GEMMs on the block shapes of the shipped model (M = 119,056 tokens), one process, the
four kernels alternating inside every repetition, HIP events, warm-up, median.  The quantiser passes are timed on their own.

    python tools/bench_gemm_mx6.py [--m 119056] [--reps 7] [--out profiles/metrics/bench_gemm_mx6.json]

FLOP/s are over the algorithmic count 2 M N K.  Inputs are hashed-uniform (synthetic.hashed_uniform).  The step time of a whole
sample_video.py run under --mxfp6-linears is not measured here."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hunyuanvideo_efficiency_amd import gemm_mx4 as mx, gemm_mx6 as mx6, ops, synthetic as syn  # noqa: E402

SHAPES = [(9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288), (21504, 3072), (3072, 15360)]     # (N, K)
BF, FP8 = torch.bfloat16, torch.float8_e4m3fn


def rows_of(m, k, key, scale, dev):
    """[m, k] bf16 on the device: a hashed-uniform block of 4096 rows, repeated down the rows (generating 1.8 G values on the host would
    take longer than the measurement)"""
    base = (syn.hashed_uniform((min(m, 4096), k), key, 5) * scale).to(BF).to(dev)
    return base.repeat((m + base.shape[0] - 1) // base.shape[0], 1)[:m].contiguous()


def timed(fns, reps, warmup=2):
    """median ms of each fn, the fns alternating inside every repetition"""
    ms = [[] for _ in fns]
    for r in range(warmup + reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[i].append(e0.elapsed_time(e1))
    return [statistics.median(v) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=119056)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics", "bench_gemm_mx6.json"))
    a = ap.parse_args()
    dev, M = "cuda", a.m
    rows = []
    for N, K in SHAPES:
        x, w = rows_of(M, K, f"bench.a{K}", 2.0, dev), rows_of(N, K, f"bench.w{N}.{K}", 0.05, dev)
        out = torch.empty(M, N, dtype=BF, device=dev)
        x8, xs = ops.quant_rows_fp8(x)
        wsc = (w.float().abs().max() / 448.0).to(BF).reshape(1)
        w8 = (w.float() / wsc.float()).clamp(-448, 448).to(FP8)
        x4, x4s = mx.quant_rows_mxfp4(x)
        w4, w4s = mx.quant_rows_mxfp4(w)
        x6, x6s = mx6.quant_rows_mxfp6(x)
        w6, w6s = mx6.quant_rows_mxfp6(w)
        t_bf, t_f8, t_mx, t_m6 = timed([lambda: ops.gemm(x, w, out=out), lambda: ops.gemm_fp8(x8, xs, w8, wsc, out=out),
                                        lambda: mx.gemm_mxfp4(x4, x4s, w4, w4s, out=out),
                                        lambda: mx6.gemm_mxfp6(x6, x6s, w6, w6s, out=out)], a.reps)
        q_f8, q_mx, q_m6 = timed([lambda: ops.quant_rows_fp8(x, out_q=x8, out_scale=xs),
                                  lambda: mx.quant_rows_mxfp4(x, codes=x4, scales=x4s),
                                  lambda: mx6.quant_rows_mxfp6(x, codes=x6, scales=x6s)], a.reps)
        fl = 2.0 * M * N * K
        row = dict(M=M, N=N, K=K, bf16_ms=t_bf, fp8_ms=t_f8, mxfp4_ms=t_mx, mxfp6_ms=t_m6, quant_rows_fp8_ms=q_f8,
                   quant_rows_mxfp4_ms=q_mx, quant_rows_mxfp6_ms=q_m6, bf16_pflops=fl / t_bf / 1e12, fp8_pflops=fl / t_f8 / 1e12,
                   mxfp4_pflops=fl / t_mx / 1e12, mxfp6_pflops=fl / t_m6 / 1e12, mxfp6_over_fp8_time=t_m6 / t_f8,
                   mxfp6_over_mxfp4_time=t_m6 / t_mx, mxfp6_over_bf16_time=t_m6 / t_bf)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, w, out, x8, w8, x4, w4, x6, w6
        torch.cuda.empty_cache()
    d = 3072
    x = rows_of(M, d, "bench.ln", 2.0, dev)
    sh, sc = (syn.hashed_uniform((d,), "bench.sh", 5) * 0.3).to(BF).to(dev), (syn.hashed_uniform((d,), "bench.sc", 5) * 0.3).to(BF).to(dev)
    o = torch.empty_like(x)
    c4, s4 = mx.ln_modulate_mxfp4(x, sh, sc)
    c8, s8 = ops.ln_modulate_fp8(x, sh, sc)
    c6, s6 = mx6.ln_modulate_mxfp6(x, sh, sc)
    ln = timed([lambda: ops.ln_modulate(x, sh, sc, out=o), lambda: ops.ln_modulate_fp8(x, sh, sc, out_q=c8, out_scale=s8),
                lambda: mx.ln_modulate_mxfp4(x, sh, sc, codes=c4, scales=s4),
                lambda: mx6.ln_modulate_mxfp6(x, sh, sc, codes=c6, scales=s6)], a.reps)
    res = dict(device=torch.cuda.get_device_name(0), method="HIP events, 2 warm-up + %d repetitions, median; kernels alternate inside a "
               "repetition; hashed-uniform inputs; FLOP/s over 2 M N K" % a.reps, gemm=rows,
               ln_modulate_ms=dict(M=M, D=d, bf16=ln[0], fp8=ln[1], mxfp4=ln[2], mxfp6=ln[3]), step_time_under_flag="not measured",
               video_fidelity_under_mxfp6="not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
