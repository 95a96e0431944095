#!/usr/bin/env python3
"""Time the adaptive tile selection of include/hv_attn_select.h and the sliding-tile kernel under the lists it writes, with HIP events: per
case --warmup rounds, then --reps rounds; a round times one launch of each step, one after the other, so all see the same machine state;
median per step.

Cases (24 heads of 128, q | k | v strided out of one fused [S, 9216] bf16 buffer of hashed-random values, 256 text rows behind the image,
tiles of (4, 8, 8)): `720p129f` grid 33 x 45 x 80, S = 119,056; `544p65f` grid 17 x 34 x 60, S = 34,936.
Steps: `dense` = hv_attn_fwd_bf16 over all S rows; `tile_3x3x3` = hv_attn_fwd_tile_bf16 under the static (3, 3, 3) window; `select_k27` =
hv_attn_select_tiles with cdf = 1, k_max = 27 (plain top-27: the key count of (3, 3, 3)), all four kernels of the pass; `tile_top27` = the
tile kernel under those lists (on hashed-random inputs the pooled scores are nearly flat, so the lists are irregular and share little between
neighbouring query tiles: what that costs in cache reuse at equal work); `copy_qk` = a device copy of the q | k image columns, the bytes the
pool kernel reads, read AND written.  `pool_bound_ms` = the read half of that copy's rate applied to the pool's bytes: the selection
pass cannot be faster.  The four kernels of the pass are not timed one by one here (one entry point enqueues them).
--synthetic-mass (CPU, no GPU needed): on the structured inputs of tests/attn_select_ref.py (random tile centres + noise: NO spatial
locality, so a geometric window is no better than chance - synthetic, and favourable to the adaptive rule by construction) the true
float64 softmax mass, token by token, that top-27 lists of the float64 rule cover, beside a (3, 3, 3) window.

Prints one JSON line per case; --out also writes them to a file (a JSON list)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("720p129f", (33, 45, 80), 256, 24), ("544p65f", (17, 34, 60), 256, 24))
TILE, K = (4, 8, 8), 27


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def synthetic_mass(grid=(10, 20, 20), tile=(2, 4, 4), H=2):
    from hunyuanvideo_efficiency_amd.attn_tile import tile_plan
    from tests import attn_select_ref as R
    base, buf, heads, _ = R.pooled(grid, tile, H)
    win = tile_plan(grid, tile, (3, 3, 3), "cpu")
    rows = [base.perm[a:b].long() for a, b in zip(base.tile_start[:-1], base.tile_start[1:])]
    cover = {"top27": [], "window_3x3x3": []}
    for h, (p, rho) in enumerate(heads):
        q, k = (buf[:, o + h * 128:o + (h + 1) * 128].double() for o in (0, H * 128))
        P = torch.softmax(q @ k.T * 128 ** -0.5, dim=1)
        per_tile = torch.stack([P[:, r].sum(1) for r in rows], 1)                 # mass of every key tile, per query token
        for i, r in enumerate(rows):
            lists = {"top27": R.cut(p[i], rho[i], i, 1.0, 1, K)[0], "window_3x3x3": win.nb_idx[win.nb_ptr[0, i]:win.nb_ptr[0, i + 1]].tolist()}
            for key, lst in lists.items():
                cover[key].append(float(per_tile[r][:, lst].sum(1).mean()))
    return {"case": "synthetic_mass", "inputs": "tests/attn_select_ref.make_inputs: random tile centres + noise, no spatial locality (synthetic)",
            "grid": list(grid), "tile": list(tile), "heads": H, "n_tiles": base.n_tiles,
            **{f"true_mass_{key}": round(statistics.mean(v), 4) for key, v in cover.items()}}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--cases", default=",".join(c[0] for c in CASES))
    p.add_argument("--synthetic-mass", action="store_true")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    lines = []
    if a.synthetic_mass:
        lines.append(synthetic_mass())
        print(json.dumps(lines[-1]), flush=True)
    elif not torch.cuda.is_available():
        raise SystemExit("bench_attn_select.py needs a GPU: a CPU run can give no time (--synthetic-mass runs without one)")
    for name, grid, n_txt, H in CASES if not a.synthetic_mass else ():
        if name not in a.cases.split(","):
            continue
        from hunyuanvideo_efficiency_amd import attn_select, ops, synthetic as syn
        dev = "cuda:0"
        n_img = grid[0] * grid[1] * grid[2]
        S, d = n_img + n_txt, H * 128
        qkv = (syn.hashed_uniform((S, 3 * d), f"bench_attn_select.{name}", 7, dev) * 3.0 ** 0.5).to(torch.bfloat16)
        q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
        o_dense, o_tile = torch.empty(S, d, dtype=torch.bfloat16, device=dev), torch.empty(S, d, dtype=torch.bfloat16, device=dev)
        qk_copy = torch.empty(n_img, 2 * d, dtype=torch.bfloat16, device=dev)
        window = ops.tile_plan(grid, TILE, (3, 3, 3), dev)
        bufs = attn_select.select_buffers(window.n_tiles, H, K, dev)
        select = lambda: attn_select.select_plan(q[:n_img], k[:n_img], H, window, 1.0, 1, K, buffers=bufs)
        top = select()
        steps = {"dense": lambda: ops.attn_fwd(q, k, v, o_dense, H),
                 "tile_3x3x3": lambda: ops.attn_fwd_tile(q[:n_img], k, v, o_tile[:n_img], H, window, dense=(n_img, S)),
                 "select_k27": select,
                 "tile_top27": lambda: ops.attn_fwd_tile(q[:n_img], k, v, o_tile[:n_img], H, top, dense=(n_img, S)),
                 "copy_qk": lambda: qk_copy.copy_(qkv[:n_img, :2 * d])}
        for _ in range(a.warmup):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        ms = {key: [] for key in steps}
        for _ in range(a.reps):
            for key, fn in steps.items():
                ms[key].append(timed(fn))
        med = {key: statistics.median(vals) for key, vals in ms.items()}
        rec = {"case": name, "grid": list(grid), "tile": list(TILE), "n_tiles": window.n_tiles, "text_rows_n": n_txt, "S": S, "heads": H,
               "warmup": a.warmup, "reps": a.reps, "k": K, "pool_bytes": n_img * 2 * d * 2}
        for key, vals in ms.items():
            rec[key] = {"ms": round(med[key], 3), "ms_min_max": [round(min(vals), 3), round(max(vals), 3)], "over_dense": round(med[key] / med["dense"], 4)}
        rec["pool_bound_ms"] = round(med["copy_qk"] / 2, 3)
        rec["select_over_pool_bound"] = round(med["select_k27"] / (med["copy_qk"] / 2), 2)
        rec["top27_over_window"] = round(med["tile_top27"] / med["tile_3x3x3"], 4)
        rec["fraction_window"], rec["fraction_top27"] = round(window.fraction, 5), round(attn_select.plan_density(top), 5)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del qkv, q, k, v, o_dense, o_tile, qk_copy, bufs, top, steps
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
