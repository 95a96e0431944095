#!/usr/bin/env python3
"""Time metrics.fvd_logits (csrc/hv_i3d.hip: preprocessing + Inception-I3D, synthetic weights) on one clip per --shape, default a
129-frame 720p fp16 clip and a 33-frame 240 x 416 one, with HIP events: warm-up, then --reps timed repetitions, median.  Per clip:
`total_ms` (the whole launch sequence, no host synchronisation inside the timed region), the convolutions' FLOP count (2 * M * Cout * K
with the true K: 3 input channels in the first layer) and the fraction of the fp32-matrix peak that is, a per-kernel split from one
extra pass with an event pair around every launch (summed per kind, and the five slowest layers), and `host_torch_fp32_ms`: the same
network (tests/i3d_ref.py, torch CPU ops, fp32) on the host for the same clip, one run - there is no GPU reference to compare with.
Prints one JSON line; --out also writes it to a file.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_metrics import timed  # noqa: E402

FP32_ROOF_TF = 157.3            # MI355X fp32-input MFMA peak


def conv_flop(T):
    """2 * M * Cout * K over the convolutions of a T x 224 x 224 input (+ the logits layer)"""
    from hunyuanvideo_efficiency_amd import metrics
    total = 0.0
    for (name, kind, ci, co, k, _, _, _), e, o, _ in metrics.i3d_walk(T, 224, 224):
        if kind == "conv":
            total += 2.0 * o[0] * o[1] * o[2] * co * (3 if name == "Conv3d_1a_7x7" else ci) * k[0] * k[1] * k[2]
        elif kind == "head":
            total += 2.0 * (e[0] - 1) * ci * co
    return total


def per_kernel(clip, model):
    """one pass with an event pair around every launch -> ({kind: ms}, [(layer, ms)] slowest first)"""
    from hunyuanvideo_efficiency_amd import _lib, metrics
    real, marks = _lib.call, []

    def call(name, *args):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        real(name, *args)
        e.record()
        marks.append((name, s, e))

    _lib.call = call
    try:
        metrics.fvd_logits(clip, model)
    finally:
        _lib.call = real
    torch.cuda.synchronize()
    kinds, layers = {}, []
    convs = [r[0] for r in metrics.I3D_LAYERS if r[1] == "conv"]
    ci = 0
    for name, s, e in marks:
        ms = s.elapsed_time(e)
        kinds[name] = kinds.get(name, 0.0) + ms
        if name == "i3d_conv3d_f32":
            layers.append((convs[ci], ms))
            ci += 1
    return kinds, sorted(layers, key=lambda t: -t[1])


def bench_clip(shape, model, warmup, reps, host):
    from hunyuanvideo_efficiency_amd import metrics
    C, T, H, W = shape
    g = torch.Generator(device="cuda:0").manual_seed(0)
    clip = (torch.rand(C, T, H, W, device="cuda:0", generator=g) * 2 - 1).half()
    med, lo, hi = timed(lambda: metrics.fvd_logits(clip, model), warmup, reps)
    flop = conv_flop(T)
    kinds, layers = per_kernel(clip, model)
    out = {"shape": list(shape), "dtype": "fp16", "total_ms": round(med, 3), "total_ms_min_max": [round(lo, 3), round(hi, 3)],
           "conv_TFLOP": round(flop / 1e12, 4), "TFps": round(flop / med / 1e9, 2), "of_roof": round(flop / med / 1e9 / FP32_ROOF_TF, 3),
           "buffers_peak_MiB": round(metrics.i3d_buffer_plan(T, 224, 224)["peak_bytes"] / 2 ** 20, 1),
           "per_kernel_ms": {k: round(v, 3) for k, v in kinds.items()}, "slowest_convs_ms": [[n, round(ms, 3)] for n, ms in layers[:5]]}
    if host:
        from tests import i3d_ref
        x = metrics.fvd_preprocess(clip).cpu()[..., :3].permute(3, 0, 1, 2).contiguous()
        sd = model.state_dict()
        with torch.no_grad():
            t0 = time.perf_counter()
            ref = i3d_ref.network(x, sd, torch.float32)
            out["host_torch_fp32_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["host_threads"] = torch.get_num_threads()
        out["max_abs_diff_vs_host_fp32"] = float((metrics.fvd_logits(clip, model).cpu() - ref).abs().max())
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--shape", type=int, nargs=4, action="append", metavar=("C", "T", "H", "W"),
                   help="repeatable; default 3 129 720 1280 and 3 33 240 416")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--no-host", action="store_true", help="skip the host torch fp32 run of the same network")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fvd.py needs a GPU: a CPU run can give no time")
    from hunyuanvideo_efficiency_amd import metrics
    model = metrics.I3D.synthetic(0)
    shapes = a.shape or [[3, 129, 720, 1280], [3, 33, 240, 416]]
    out = {"metric": metrics.FVD_LABEL, "weights": "synthetic", "warmup": a.warmup, "reps": a.reps, "fp32_roof_TF": FP32_ROOF_TF,
           "clips": [bench_clip(s, model, a.warmup, a.reps, not a.no_host) for s in shapes]}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
