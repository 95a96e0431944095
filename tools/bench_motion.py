#!/usr/bin/env python3
"""Time the block-matching motion kernel (csrc/hv_motion.hip, hv_block_motion) with HIP events: warm-up, then --reps timed windows of
--inner launches each, median per launch.  Two shapes - a 129-frame 720p fp16 clip and a 33-frame 240 x 416 fp16 clip -, two geometries -
(block, radius) = (16, 16) and (8, 8) - and three inputs each:

  * `random`    uniform noise: every candidate is about as bad as any other;
  * `constant`  one value everywhere: every candidate ties, (0, 0) wins by the norm;
  * `pan`       a smooth random texture that moves by one pixel a frame: what a slow camera pan looks like.

The search is exhaustive and has no early exit, so the time should not depend on the content; `spread` (max / min of the three medians)
after the cases of a geometry reports what was measured - a data-dependent time would be a finding.

Per case: `ms`, `byte_diffs` = pairs x blocks x (2 R + 1)^2 x block^2 (partial blocks counted whole: the kernel spends the instructions),
`Tdiffs_per_s` and `share_of_sad_issue_bound`: the bound is one v_sad_u8 (four byte differences per lane) per wave every 2 cycles on each of
the 4 SIMDs of 256 CUs at 2.4 GHz = 128 x 4 x 256 x 2.4e9 = 314.6e12 byte differences a second (the micro-architecture guide: "A wave (64
lanes) is assigned to one SIMD and issues each VALU instruction over 2 cycles (32 lanes/cycle x 2)"; 256 CUs, 4 SIMDs per CU, 2400 MHz).
`host_numpy_s`: the numpy restatement tests/motion_ref.py on this machine's CPU for the same clip - it times --host-pairs frame pairs and
scales to the clip's T - 1 (`host_pairs_timed` says how many; --no-host skips it) - and `fields_equal_host`: those pairs' rows against the
device's, bit for bit.

Prints one JSON line per case; --out also writes them to a file (a JSON list).  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAD_ISSUE_BOUND = 128 * 4 * 256 * 2.4e9          # byte differences per second, see above
SHAPES = (("720p129f", (3, 129, 720, 1280)), ("240p33f", (3, 33, 240, 416)))
GEOMETRIES = ((16, 16), (8, 8))
INPUTS = ("random", "constant", "pan")


def make_input(kind, shape, dev):
    C, T, H, W = shape
    g = torch.Generator(device=dev).manual_seed(0)
    if kind == "random":
        return (torch.rand(shape, device=dev, generator=g) * 2 - 1).to(torch.float16)
    if kind == "constant":
        return torch.full(shape, 0.25, dtype=torch.float16, device=dev)
    tex = torch.rand(1, 1, H // 8 + 2, (W + T) // 8 + 2, device=dev, generator=g) * 1.6 - 0.8
    tex = torch.nn.functional.interpolate(tex, scale_factor=8, mode="bilinear", align_corners=False)[0, 0]
    frames = torch.stack([tex[:H, t:t + W] for t in range(T)])                      # one pixel to the left per frame
    return frames[None].expand(3, T, H, W).to(torch.float16).contiguous()


def timed(fn, warmup, reps, inner):
    """median / min / max ms of ONE call of fn, from `reps` event windows of `inner` calls each"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ms), min(ms), max(ms)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=3, help="launches per timed window")
    p.add_argument("--no-host", action="store_true", help="skip the host numpy pass")
    p.add_argument("--host-pairs", type=int, default=1, help="frame pairs the host pass times before scaling to the clip")
    p.add_argument("--only", type=str, default=None, help="run one shape by name")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import _lib, metrics
    from tests import motion_ref
    dev = "cuda:0"
    luma = metrics.GRAY_LUMA
    lines = []
    for sname, shape in SHAPES:
        if a.only and a.only != sname:
            continue
        C, T, H, W = shape
        for block, radius in GEOMETRIES:
            lam = metrics.motion_default_lam(block)
            Hb, Wb = -(-H // block), -(-W // block)
            mv = torch.empty(T - 1, Hb, Wb, 2, dtype=torch.int16, device=dev)
            sad = torch.empty(T - 1, Hb, Wb, dtype=torch.int32, device=dev)
            sad0 = torch.empty_like(sad)
            diffs = (T - 1) * Hb * Wb * (2 * radius + 1) ** 2 * block * block
            by_kind = {}
            for kind in INPUTS:
                x = make_input(kind, shape, dev)

                def run():
                    _lib.call("block_motion", x, x.stride(0), x.stride(1), x.stride(2), 0, T, H, W, 1, *luma, block, radius, lam, mv, sad, sad0)
                med, lo, hi = timed(run, a.warmup, a.reps, a.inner)
                stats = metrics.motion_stats(x, block, radius, lam)
                out = {"case": f"{sname}_b{block}r{radius}_{kind}", "shape": list(shape), "dtype": "float16", "input": kind, "block": block,
                       "radius": radius, "lam": lam, "warmup": a.warmup, "reps": a.reps, "inner": a.inner, "ms": round(med, 4),
                       "ms_min_max": [round(lo, 4), round(hi, 4)], "byte_diffs": diffs, "Tdiffs_per_s": round(diffs / med / 1e9, 2),
                       "share_of_sad_issue_bound": round(diffs / (med * 1e-3) / SAD_ISSUE_BOUND, 4), "motion_mean": stats["motion_mean"],
                       "static_share": stats["static_share"], "mc_gain": stats["mc_gain"]}
                if not a.no_host:
                    n = min(a.host_pairs, T - 1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    want = motion_ref.block_motion(x[:, :n + 1].float().cpu().numpy(), block, radius, lam)
                    dt = time.perf_counter() - t0
                    out["host_pairs_timed"], out["host_numpy_s"] = n, round(dt / n * (T - 1), 2)
                    out["host_over_device"] = round(dt / n * (T - 1) * 1e3 / med, 1)
                    got = (mv[:n].cpu().numpy(), sad[:n].cpu().numpy(), sad0[:n].cpu().numpy())
                    out["fields_equal_host"] = bool(all((g_ == w_.astype(g_.dtype)).all() for g_, w_ in zip(got, want)))
                by_kind[kind] = med
                print(json.dumps(out), flush=True)
                lines.append(out)
                del x
                torch.cuda.empty_cache()
            spread = {"case": f"{sname}_b{block}r{radius}_spread", "spread": round(max(by_kind.values()) / min(by_kind.values()), 3),
                      "ms": {k: round(v, 4) for k, v in by_kind.items()}}
            print(json.dumps(spread), flush=True)
            lines.append(spread)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
