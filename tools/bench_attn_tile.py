#!/usr/bin/env python3
"""Time the sliding-tile attention of include/hv_attn_tile.h beside the dense bf16 kernel, with HIP events: per case --warmup rounds, then
--reps rounds; a round times one launch of each kernel, one after the other, so all see the same machine state; median per launch.

Cases (24 heads of 128, q | k | v strided out of one fused [S, 9216] bf16 buffer of hashed-random values, 256 text rows behind the image):
  * `720p129f`  grid 33 x 45 x 80, S = 119,056 (the flagship step's main segment);
  * `544p65f`   grid 17 x 34 x 60, S = 34,936.
Launches: `dense` = hv_attn_fwd_bf16 over all S rows (with its workspace, as the model calls it); `tile_3x3x3`, `tile_3x3x5` and
`tile_full` = hv_attn_fwd_tile_bf16 over the image rows with tiles of (4, 8, 8), the window named (full: a window over the whole tile
grid, the FLOPs of dense image attention - what the gather and the ragged tiles cost) and the text as dense range; `text_rows` = the dense
kernel for the 256 text queries against all keys, the second launch of the model's sliding-tile segment.
Per launch: `ms`, its spread, `fraction` (attended image keys per image query, from the plan), `TFLOPs` = 4 * 128 * H * (query, key) pairs
actually computed / ms, `over_dense` = ms / dense ms (below 1: faster), and for the tile launches `segment_over_dense` with the text rows'
launch added.  `max_abs_full_vs_dense` is the distance of the full-window output from the dense kernel's on the image rows.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("720p129f", (33, 45, 80), 256, 24), ("544p65f", (17, 34, 60), 256, 24))
TILE = (4, 8, 8)


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
        raise SystemExit("bench_attn_tile.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import ops, synthetic as syn
    dev = "cuda:0"
    lines = []
    for name, grid, n_txt, H in CASES:
        if name not in a.cases.split(","):
            continue
        n_img = grid[0] * grid[1] * grid[2]
        S, d = n_img + n_txt, H * 128
        qkv = (syn.hashed_uniform((S, 3 * d), f"bench_attn_tile.{name}", 7, dev) * 3.0 ** 0.5).to(torch.bfloat16)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        o_dense, o_tile = torch.empty(S, d, dtype=torch.bfloat16, device=dev), torch.empty(S, d, dtype=torch.bfloat16, device=dev)
        full = tuple(-(-g // t) for g, t in zip(grid, TILE))
        plans = {"tile_3x3x3": ops.tile_plan(grid, TILE, (3, 3, 3), dev), "tile_3x3x5": ops.tile_plan(grid, TILE, (3, 3, 5), dev),
                 "tile_full": ops.tile_plan(grid, TILE, full, dev)}
        steps = {"dense": lambda: ops.attn_fwd(q, k, v, o_dense, H)}
        for key, plan in plans.items():
            steps[key] = lambda plan=plan: ops.attn_fwd_tile(q[:n_img], k, v, o_tile[:n_img], H, plan, dense=(n_img, S))
        steps["text_rows"] = lambda: ops.attn_fwd(q[n_img:], k, v, o_tile[n_img:], H)
        for _ in range(a.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        ms = {key: [] for key in steps}
        for _ in range(a.reps):
            for key, fn in steps.items():
                ms[key].append(timed(fn))
        pairs = {"dense": float(S) * S, "text_rows": float(n_txt) * S}
        pairs.update({key: n_img * (plan.fraction * n_img + n_txt) for key, plan in plans.items()})
        rec = {"case": name, "grid": list(grid), "tile": list(TILE), "text_rows_n": n_txt, "S": S, "heads": H, "warmup": a.warmup, "reps": a.reps}
        med = {key: statistics.median(vals) for key, vals in ms.items()}
        for key, vals in ms.items():
            rec[key] = {"ms": round(med[key], 3), "ms_min_max": [round(min(vals), 3), round(max(vals), 3)],
                        "TFLOPs": round(4.0 * 128 * H * pairs[key] / med[key] / 1e9, 1), "over_dense": round(med[key] / med["dense"], 4)}
            if key in plans:
                rec[key].update(window=list(plans[key].windows[0]), fraction=round(plans[key].fraction, 5),
                                segment_over_dense=round((med[key] + med["text_rows"]) / med["dense"], 4))
        steps["dense"](), steps["tile_full"]()
        rec["max_abs_full_vs_dense"] = round(max(float((o_tile[r0:r0 + 8192].float() - o_dense[r0:r0 + 8192].float()).abs().max())
                                                 for r0 in range(0, n_img, 8192)), 6)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del qkv, q, k, v, o_dense, o_tile, plans, steps
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
