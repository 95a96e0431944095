#!/usr/bin/env python3
"""Time the linear temporal interpolation (csrc/hv_temporal.hip, hv_temporal_interp_f16) with HIP events and, on the same shapes in the
same process, the nearest mode it stands beside (hv_temporal_resample_f16, mode 1): warm-up, then --reps rounds; a round times a window
of --inner launches of one kernel and then of the other, so both see the same machine state; median per launch.

Kernel shapes (fp16, channels-last [T, HW, C], scale factor 2):
  * `240p33f_up3`   the 128-channel activation of the last up block for a 240 x 416 clip, 17 frames in, 34 out;
  * `720p_tile_up3` the same for the largest spatial tile of a 720p decode (256 x 256 samples), 17 frames in, 34 out.
Per kernel: `ms`, `hbm_bytes` = what the algorithm must move (the input once, the output once), `GBps` = hbm_bytes / ms and its share of
the 6.3 TB/s a streaming copy reaches on these machines (README.md); `linear_over_nearest`, the ratio of the two times, beside
`bytes_ratio_min` = (1 + s) / (1 + s) = 1 (every source frame read once) and `bytes_ratio_max` = (2 s + s) / (1 + s) (two source frames
read per output frame, nothing shared) - where the time ratio is above 1 the rest is what the kernel adds to a copy.

Study level (--study; synthetic weights, the full 884 topology), one line each:
  * `ae_240p65f`    auto-encoder forward of a 240 x 416 x 65-frame clip under one pool (encoder block 0) and one x2 interpolation of the
                    128-channel activation (decoder block 3), with interp_mode "trilinear" and with "nearest": `trilinear_s`, `nearest_s`;
  * `ae_720p33f_tiled`  a 720 x 1280 x 33-frame clip under the same configuration with spatial tiling: `trilinear_s`.  It has no
                    earlier figure: before spatial tiling was allowed under t_ops the VAE refused this call.

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

COPY_ROOF_TBPS = 6.3            # streaming-copy rate measured on these machines (README.md)
SHAPES = (("240p33f_up3", 17, 240 * 416, 128, 2), ("720p_tile_up3", 17, 256 * 256, 128, 2))


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def t_ops(mode):
    return {"encoder": {"down_blocks": [{"block_index": 0, "pool_t_kernel": 3, "pool_t_stride": 2, "enable_t_pool_before_block": [False, True],
                                         "enable_t_pool_after_block": [False, False]}]},
            "decoder": {"up_blocks": [{"block_index": 3, "enable_t_interp_before_block": [False, False, False],
                                       "enable_t_interp_after_block": [True, False, False], "interp_t_scale_factor": 2, "interp_mode": mode}]}}


def forward_s(vae, x, reps):
    vae(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        y = vae(x).sample
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), list(y.shape)


def study(reps, dev):
    from hunyuanvideo_efficiency_amd import synthetic as syn
    from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D
    boc = syn.VAE_BLOCK_OUT_CHANNELS
    vae = AutoencoderKLCausal3D(block_out_channels=boc, device=dev, with_encoder=True)
    vae.load_state_dict({k: v.to(torch.float16) for k, v in syn.synth_vae_state_dict(boc, seed=0, encoder=True).items()}, strict=True)
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.rand((1, 3, 65, 240, 416), device=dev, generator=g) * 2 - 1).to(torch.float16)
    out = {"case": "ae_240p65f", "clip": list(x.shape), "reps": reps}
    for mode in ("trilinear", "nearest", "trilinear", "nearest"):          # alternating: the second pass of each is the one reported
        vae.apply_t_ops_config(t_ops(mode))
        out[mode + "_s"], out["recon"] = forward_s(vae, x, reps)
    out = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}
    out["trilinear_over_nearest"] = round(out["trilinear_s"] / out["nearest_s"], 4)
    yield out
    del x
    torch.cuda.empty_cache()
    x = (torch.rand((1, 3, 33, 720, 1280), device=dev, generator=g) * 2 - 1).to(torch.float16)
    vae.apply_t_ops_config(t_ops("trilinear"))
    vae.enable_spatial_tiling()
    s, shape = forward_s(vae, x, reps)
    yield {"case": "ae_720p33f_tiled", "clip": list(x.shape), "reps": reps, "tiling": "spatial", "trilinear_s": round(s, 4), "recon": shape}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--inner", type=int, default=50, help="launches per timed window")
    p.add_argument("--study", action="store_true", help="also the two auto-encoder lines")
    p.add_argument("--study-reps", type=int, default=3)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tinterp.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import _lib
    dev = "cuda:0"
    lines = []
    for name, T, HW, C, s in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = (torch.rand((T * HW, C), device=dev, generator=g) * 2 - 1).to(torch.float16)
        out_l = torch.empty(T * s * HW, C, dtype=torch.float16, device=dev)
        out_n = torch.empty_like(out_l)

        def linear():
            _lib.call("temporal_interp_f16", x, C, out_l, C, T, HW, C, s)

        def nearest():
            _lib.call("temporal_resample_f16", x, C, out_n, C, T, HW, C, 1, 1, s)
        for _ in range(a.warmup):
            linear(), nearest()
        torch.cuda.synchronize()
        ms = {"linear": [], "nearest": []}
        for _ in range(a.reps):
            ms["linear"].append(window(linear, a.inner))
            ms["nearest"].append(window(nearest, a.inner))
        hbm = (x.numel() + out_l.numel()) * 2
        rec = {"case": name, "shape": [T, HW, C], "scale": s, "dtype": "float16", "warmup": a.warmup, "reps": a.reps, "inner": a.inner,
               "hbm_bytes": hbm, "bytes_ratio_min": 1.0, "bytes_ratio_max": round(3 * s / (1 + s), 3)}
        for k, v in ms.items():
            med = statistics.median(v)
            rec[k] = {"ms": round(med, 4), "ms_min_max": [round(min(v), 4), round(max(v), 4)], "GBps": round(hbm / med / 1e6, 1),
                      "share_of_copy_rate": round(hbm / med / 1e9 / COPY_ROOF_TBPS, 3)}
        rec["linear_over_nearest"] = round(rec["linear"]["ms"] / rec["nearest"]["ms"], 3)
        # the copies among the linear outputs are the nearest mode's frames: the two kernels agree there bit for bit
        rec["clamped_ends_equal_nearest"] = bool(torch.equal(out_l[:HW], out_n[:HW]) and torch.equal(out_l[-HW:], out_n[-HW:]))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, out_l, out_n
        torch.cuda.empty_cache()
    if a.study:
        for rec in study(a.study_reps, dev):
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return lines


if __name__ == "__main__":
    main()
