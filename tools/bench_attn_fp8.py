#!/usr/bin/env python3
"""Time the FP8 attention of include/hv_attn_fp8.h beside the bf16 kernel it stands next to, with HIP events: per case --warmup rounds,
then --reps rounds; a round times one launch of hv_attn_fwd_bf16 (with its workspace), one of hv_attn_fp8_quantise and one of
hv_attn_fwd_fp8, one after the other, so all three see the same machine state; median per launch.

Cases (24 heads of 128, q | k | v strided out of one fused [S, 9216] bf16 buffer of hashed-random values, n_q = n_kv = S):
  * `720p129f`  S = 119,056 (the flagship step's main segment);
  * `544p129f`  S = 34,936.
Per kernel: `ms`, its spread, and for the two attention kernels `PFLOPs` = 4 S^2 128 H / ms (the FLOPs of the two products).  For the
quantiser `hbm_bytes` = what it must move (K and V read twice, Q once, the codes written once) and `GBps`.  `fp8_total_ms` = quantise +
forward, `fp8_total_over_bf16` their ratio to the bf16 kernel (below 1: FP8 wins), `fp8_fwd_over_bf16` the main loops alone.  `max_abs`
and `rms` are the distance of the FP8 output from the bf16 kernel's on the same inputs, beside `out_rms`.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("720p129f", 119056, 24), ("544p129f", 34936, 24))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cases", default=",".join(c[0] for c in CASES))
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_fp8.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import ops, synthetic as syn
    dev = "cuda:0"
    lines = []
    for name, S, H in CASES:
        if name not in a.cases.split(","):
            continue
        d = H * 128
        qkv = (syn.hashed_uniform((S, 3 * d), f"bench_attn_fp8.{name}", 7, dev) * 3.0 ** 0.5).to(torch.bfloat16)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        o16, o8 = torch.empty(S, d, dtype=torch.bfloat16, device=dev), torch.empty(S, d, dtype=torch.bfloat16, device=dev)
        ws = torch.empty(ops.attn_fp8_workspace_bytes(S, S, H), dtype=torch.uint8, device=dev)
        from hunyuanvideo_efficiency_amd import _lib
        steps = {"bf16": lambda: ops.attn_fwd(q, k, v, o16, H),
                 "fp8_quantise": lambda: ops.attn_fp8_quantise(q, k, v, H, workspace=ws),
                 "fp8_fwd": lambda: _lib.call("attn_fwd_fp8", ws, ws.numel(), o8, d, S, S, H, 128)}
        for _ in range(a.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        ms = {key: [] for key in steps}
        for _ in range(a.reps):
            for key, fn in steps.items():
                ms[key].append(timed(fn))
        flops = 4.0 * S * S * 128 * H
        hbm = (2 * 2 * S * d + S * d) * 2 + 3 * S * d
        rec = {"case": name, "S": S, "heads": H, "warmup": a.warmup, "reps": a.reps, "workspace_bytes": ws.numel()}
        for key, vals in ms.items():
            med = statistics.median(vals)
            rec[key] = {"ms": round(med, 3), "ms_min_max": [round(min(vals), 3), round(max(vals), 3)]}
            if key == "fp8_quantise":
                rec[key].update(hbm_bytes=hbm, GBps=round(hbm / med / 1e6, 1))
            else:
                rec[key]["PFLOPs"] = round(flops / med / 1e12, 3)
        rec["fp8_total_ms"] = round(rec["fp8_quantise"]["ms"] + rec["fp8_fwd"]["ms"], 3)
        rec["fp8_total_over_bf16"] = round(rec["fp8_total_ms"] / rec["bf16"]["ms"], 3)
        rec["fp8_fwd_over_bf16"] = round(rec["fp8_fwd"]["ms"] / rec["bf16"]["ms"], 3)
        diff = torch.zeros((), dtype=torch.float64, device=dev)
        sq = torch.zeros((), dtype=torch.float64, device=dev)
        mx = 0.0
        for r0 in range(0, S, 8192):                # by row blocks: no second S x d fp32 buffer
            e = o8[r0:r0 + 8192].float() - o16[r0:r0 + 8192].float()
            mx = max(mx, float(e.abs().max()))
            diff += (e.double() ** 2).sum()
            sq += (o16[r0:r0 + 8192].double() ** 2).sum()
        rec.update(max_abs=round(mx, 6), rms=round(float((diff / (S * d)).sqrt()), 6), out_rms=round(float((sq / (S * d)).sqrt()), 6))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del qkv, q, k, v, o16, o8, ws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
