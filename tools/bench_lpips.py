#!/usr/bin/env python3
"""Time the LPIPS (AlexNet) scoring kernels (csrc/hv_lpips.hip) on one video pair, default 3 x 129 x 720 x 1280 fp16, synthetic weights,
with HIP events: warm-up, then --reps timed repetitions, median.  Each kernel is timed on one chunk of frames (the chunk
metrics.lpips_video picks by default, both videos in one launch) with the previous kernel's output as its input: the five conv layers
(ms, and TF/s = 2 * M * Cout * K / time with the true K, 363 for the first layer), the two pools, the five layer distances.  `total` is
the whole clip through metrics.lpips_video's launch sequence (every chunk, no host synchronisation inside the timed region).  Prints
one JSON line; --out also writes it to a file.  Needs a GPU."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402

FP32_ROOF_TF = 157.3            # MI355X fp32 vector / fp32-input MFMA peak


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=4, default=[3, 129, 720, 1280], metavar=("C", "T", "H", "W"))
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--frames-per-chunk", type=int, default=None)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import _lib, metrics
    C, T, H, W = a.shape
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    ref = (torch.rand(C, T, H, W, device=dev, generator=g) * 2 - 1).half()
    rec = (ref.float() + 0.05 * torch.randn(C, T, H, W, device=dev, generator=g)).half()
    model = metrics.LpipsAlex.synthetic(0)
    wts = model.on(dev)
    sizes = metrics.lpips_map_sizes(H, W)
    pixels, _, default_chunk = metrics.lpips_buffer_plan(H, W)
    Tc = min(a.frames_per_chunk or default_chunk, T)
    N = 2 * Tc
    out = {"shape": [C, T, H, W], "dtype": "fp16", "weights": "synthetic", "frames_per_chunk": Tc, "images_per_launch": N,
           "warmup": a.warmup, "reps": a.reps, "fp32_roof_TF": FP32_ROOF_TF, "map_sizes": sizes}

    # one buffer per stage, so that every kernel can be repeated on an unchanging input
    feats = [torch.empty(N * px * c, dtype=torch.float32, device=dev) for px, c in zip(pixels, metrics.LPIPS_CHNS)]
    pooled = [torch.empty(N * pixels[1] * 64, dtype=torch.float32, device=dev), torch.empty(N * pixels[2] * 192, dtype=torch.float32, device=dev)]
    sums = torch.empty(Tc, 5, dtype=torch.float64, device=dev)
    ws = torch.empty(max(_lib.host("lpips_distance_workspace_bytes", Tc, pixels[0]), 16), dtype=torch.uint8, device=dev)
    va, vr = ref[:, :Tc], rec[:, :Tc]

    def conv(layer):
        _, ci, co, k, _, pad = metrics.LPIPS_CONVS[layer]
        if layer == 0:
            _lib.call("lpips_conv1_f32", va, va.stride(0), va.stride(1), va.stride(2), vr, vr.stride(0), vr.stride(1), vr.stride(2), 0, Tc, H, W,
                      1, wts["lut"], wts["w"][0], wts["b"][0], feats[0])
        else:
            src = pooled[layer - 1] if layer <= 2 else feats[layer - 1]
            _lib.call("lpips_conv2d_f32", src, wts["w"][layer], wts["b"][layer], feats[layer], N, sizes[layer][0], sizes[layer][1], ci, co, k, pad)

    def pool(i):
        _lib.call("lpips_maxpool_f32", feats[i], pooled[i], N, sizes[i][0], sizes[i][1], metrics.LPIPS_CHNS[i])

    def dist(layer):
        _lib.call("lpips_distance_f32", feats[layer], wts["lin"][layer], Tc, pixels[layer], metrics.LPIPS_CHNS[layer], layer, sums, ws, ws.numel())

    chunk_ms = 0.0
    conv_flop = 0.0
    for layer in range(5):
        _, ci, co, k, _, _ = metrics.LPIPS_CONVS[layer]
        med, lo, hi = timed(lambda: conv(layer), a.warmup, a.reps)
        flop = 2.0 * N * pixels[layer] * co * ci * k * k
        conv_flop += flop
        out[f"conv{layer + 1}_ms"] = round(med, 4)
        out[f"conv{layer + 1}_ms_min_max"] = [round(lo, 4), round(hi, 4)]
        out[f"conv{layer + 1}_TFps"] = round(flop / med / 1e9, 2)
        out[f"conv{layer + 1}_of_roof"] = round(flop / med / 1e9 / FP32_ROOF_TF, 3)
        chunk_ms += med
        if layer < 2:
            med, lo, hi = timed(lambda: pool(layer), a.warmup, a.reps)
            out[f"pool{layer + 1}_ms"] = round(med, 4)
            out[f"pool{layer + 1}_GBps"] = round((feats[layer].numel() + pooled[layer].numel()) * 4 / med / 1e6, 1)
            chunk_ms += med
        med, lo, hi = timed(lambda: dist(layer), a.warmup, a.reps)
        out[f"dist{layer + 1}_ms"] = round(med, 4)
        out[f"dist{layer + 1}_GBps"] = round(feats[layer].numel() * 4 / med / 1e6, 1)
        chunk_ms += med
    out["chunk_kernels_ms"] = round(chunk_ms, 4)
    out["conv_TFps_all_layers"] = round(conv_flop / sum(out[f"conv{i}_ms"] for i in range(1, 6)) / 1e9, 2)
    del feats, pooled
    med, lo, hi = timed(lambda: metrics._lpips_enqueue(ref, rec, model, True, a.frames_per_chunk), a.warmup, a.reps)
    out["total_ms"] = round(med, 3)
    out["total_ms_min_max"] = [round(lo, 3), round(hi, 3)]
    out["total_conv_TFLOP"] = round(conv_flop * T / Tc / 1e12, 3)
    out["total_TFps"] = round(conv_flop * T / Tc / med / 1e9, 2)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
