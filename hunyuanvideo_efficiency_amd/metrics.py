"""PSNR / SSIM of a reconstruction against its input, scored on the device (csrc/hv_metrics.hip).

The fork's study scores reconstructions with evaluation/compute_metrics.py: per frame `compute_psnr` / `compute_ssim` (skimage) on
the 8-bit frames of an mp4 that `save_videos_grid(..., rescale=True)` wrote, averaged over all frames of an experiment.  Here the
same per-frame numbers come from one kernel call on the fp16 tensors still on the card: quantisation to 8 bits in registers (bit for
bit `utils.file_utils.frames_uint8`), exact integer moments, and the host rules of the reference on top (`scores_from_stats`).
What it is not: there is no video codec in between (the reference's frames went through libx264), and there is no LPIPS (it needs
AlexNet + LPIPS weights; result files carry no `LPIPS` key).  CPU tensors are refused like everywhere else in the package."""
from __future__ import annotations

import math
import os
from datetime import datetime

import numpy as np
import torch

from . import _lib

WIN = 7                     # skimage.metrics.structural_similarity default window


def scores_from_stats(sse, minmax, ssim_sum, C: int, H: int, W: int):
    """Host rules of evaluation/compute_metrics.py:31-41 on the kernel's per-frame statistics (numpy, float64).
    sse [T] int64, minmax [T,4] (min1, max1, min2, max2), ssim_sum [T,C] -> (psnr [T], ssim [T])."""
    sse = np.asarray(sse, dtype=np.int64)
    minmax = np.asarray(minmax)
    ssim_sum = np.asarray(ssim_sum, dtype=np.float64)
    psnr = np.empty(sse.shape[0], dtype=np.float64)
    ssim = np.empty(sse.shape[0], dtype=np.float64)
    npos = (H - WIN + 1) * (W - WIN + 1)
    for t in range(sse.shape[0]):
        mse = float(sse[t]) / float(C * H * W) / 255.0 ** 2
        psnr[t] = 100.0 if mse < 1.0e-10 else 20.0 * math.log10(1.0 / math.sqrt(mse))
        if minmax[t, 0] == minmax[t, 1] or minmax[t, 2] == minmax[t, 3]:
            ssim[t] = 1.0                                   # either frame constant
        else:
            ssim[t] = float(np.mean(ssim_sum[t] / npos))
    return psnr, ssim


_DTYPES = {torch.float16: 0, torch.float32: 1}


def _check_video(x: torch.Tensor, name: str):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.HVKernelError(f"{name}: expected a GPU tensor (this package has no CPU path), got "
                                 f"{x.device if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dtype not in _DTYPES:
        raise _lib.HVKernelError(f"{name}: the metrics kernel reads fp16 or fp32, got {x.dtype}")
    if x.dim() not in (4, 5):
        raise _lib.HVKernelError(f"{name}: expected [C,T,H,W] or [B,C,T,H,W], got {tuple(x.shape)}")
    if x.stride(-1) != 1 and x.shape[-1] > 1:
        raise _lib.HVKernelError(f"{name}: the W dimension must be contiguous (strides {x.stride()})")


def video_stats(ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True) -> dict:
    """Raw per-frame statistics, left on the device: `sse` int64 [B,T], `minmax` int32 [B,T,4] (min/max of ref, min/max of rec over the
    8-bit frame), `ssim_sum` float64 [B,T,C]; [C,T,H,W] inputs count as B = 1.  Scores the first min(T_ref, T_rec) frames (the
    reference zips the two frame lists).  Nothing is synchronised."""
    _check_video(ref, "ref"), _check_video(rec, "rec")
    if ref.dim() == 4:
        ref = ref[None]
    if rec.dim() == 4:
        rec = rec[None]
    if ref.dtype != rec.dtype:
        raise _lib.HVKernelError(f"ref and rec must have one dtype, got {ref.dtype} and {rec.dtype}")
    if ref.device != rec.device:
        raise _lib.HVKernelError(f"ref and rec are on different devices: {ref.device}, {rec.device}")
    B, C, _, H, W = ref.shape
    if (rec.shape[0], rec.shape[1], rec.shape[3], rec.shape[4]) != (B, C, H, W):
        raise _lib.HVKernelError(f"ref {tuple(ref.shape)} and rec {tuple(rec.shape)} differ in more than the frame count")
    T = min(ref.shape[2], rec.shape[2])
    dev = ref.device
    sse = torch.empty(B, T, dtype=torch.int64, device=dev)
    minmax = torch.empty(B, T, 4, dtype=torch.int32, device=dev)
    ssim_sum = torch.empty(B, T, C, dtype=torch.float64, device=dev)
    ws_bytes = _lib.host("video_metrics_workspace_bytes", C, T, H, W)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    for b in range(B):                        # one stream: the launches of video b + 1 reuse the workspace after video b's folds
        a, r = ref[b], rec[b]
        _lib.call("video_metrics", a, a.stride(0), a.stride(1), a.stride(2), r, r.stride(0), r.stride(1), r.stride(2),
                  _DTYPES[ref.dtype], C, T, H, W, 1 if rescale else 0, 3, sse[b], minmax[b], ssim_sum[b], ws, ws.numel())
    return {"sse": sse, "minmax": minmax, "ssim_sum": ssim_sum, "shape": (B, C, T, H, W)}


def video_metrics(ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True) -> dict:
    """PSNR / SSIM per frame of `rec` against `ref` ([C,T,H,W] or [B,C,T,H,W] GPU tensors, fp16 or fp32, values in [-1, 1] with
    rescale=True, [0, 1] without).  One host synchronisation.  Returns float64 numpy arrays `psnr`, `ssim` ([T], or [B,T] for a batch),
    their means `psnr_mean`, `ssim_mean`, and the raw integers `sse`, `minmax` the scores were formed from."""
    batched = ref.dim() == 5
    st = video_stats(ref, rec, rescale)
    B, C, T, H, W = st["shape"]
    host = {}
    for k in ("sse", "minmax", "ssim_sum"):
        host[k] = torch.empty(st[k].shape, dtype=st[k].dtype, pin_memory=True)
        host[k].copy_(st[k], non_blocking=True)
    torch.cuda.current_stream(ref.device).synchronize()
    sse, minmax, ssim_sum = (host[k].numpy().copy() for k in ("sse", "minmax", "ssim_sum"))
    psnr = np.empty((B, T), dtype=np.float64)
    ssim = np.empty((B, T), dtype=np.float64)
    for b in range(B):
        psnr[b], ssim[b] = scores_from_stats(sse[b], minmax[b], ssim_sum[b], C, H, W)
    if not batched:
        psnr, ssim, sse, minmax, ssim_sum = psnr[0], ssim[0], sse[0], minmax[0], ssim_sum[0]
    return {"psnr": psnr, "ssim": ssim, "psnr_mean": float(psnr.mean()), "ssim_mean": float(ssim.mean()),
            "sse": sse, "minmax": minmax, "ssim_sum": ssim_sum}


def save_results(results: dict, root1: str, root2: str, results_dir: str, timestamp: str = None) -> str:
    """evaluation/compute_metrics.py:73-85: metrics_<timestamp>.txt with the reference's lines."""
    os.makedirs(results_dir, exist_ok=True)
    timestamp = timestamp or datetime.now().strftime("%Y%m%d_%H%M%S")
    path = os.path.join(results_dir, f"metrics_{timestamp}.txt")
    with open(path, "w") as f:
        f.write("\n")
        f.write(f"Root1: {root1}\n")
        f.write(f"Root2: {root2}\n")
        f.write(f"Timestamp: {timestamp}\n")
        for metric, value in results.items():
            f.write(f"{metric}: {value}\n")
        f.write("\n")
    return path


class MetricsAccumulator:
    """Per-frame scores of many videos; the experiment's number is the mean over all FRAMES (compute_metrics.py:150-154), so a long
    video weighs more than a short one."""

    def __init__(self):
        self.psnr, self.ssim = [], []

    def add(self, psnr, ssim):
        """per-frame arrays of one video (or a [B,T] batch), e.g. video_metrics(...)["psnr"], ["ssim"]"""
        psnr, ssim = np.asarray(psnr, dtype=np.float64).ravel(), np.asarray(ssim, dtype=np.float64).ravel()
        if psnr.shape != ssim.shape:
            raise ValueError(f"psnr has {psnr.size} frames, ssim {ssim.size}")
        self.psnr.extend(psnr.tolist())
        self.ssim.extend(ssim.tolist())

    def add_video(self, ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True) -> dict:
        m = video_metrics(ref, rec, rescale)
        self.add(m["psnr"], m["ssim"])
        return m

    @property
    def frames(self) -> int:
        return len(self.psnr)

    def result(self) -> dict:
        """{"PSNR": ..., "SSIM": ...}; empty when nothing was added (the reference writes no key then)."""
        out = {}
        if self.psnr:
            out["PSNR"] = sum(self.psnr) / len(self.psnr)
            out["SSIM"] = sum(self.ssim) / len(self.ssim)
        return out

    def save(self, results_dir: str, root1: str, root2: str, timestamp: str = None) -> str:
        return save_results(self.result(), root1, root2, results_dir, timestamp)
