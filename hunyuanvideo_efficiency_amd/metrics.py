"""PSNR / SSIM / LPIPS of a reconstruction against its input, temporal spectra, FVD and content statistics, on the device
(csrc/hv_metrics.hip, hv_lpips.hip, hv_spectrum.hip, hv_i3d.hip, hv_content.hip).

The fork's study scores reconstructions with evaluation/compute_metrics.py: per frame `compute_psnr` / `compute_ssim` (skimage) on
the 8-bit frames of an mp4 that `save_videos_grid(..., rescale=True)` wrote, averaged over all frames of an experiment.  Here the
same per-frame numbers come from one kernel call on the fp16 tensors still on the card: quantisation to 8 bits in registers (bit for
bit `utils.file_utils.frames_uint8`), exact integer moments, and the host rules of the reference on top (`scores_from_stats`).
LPIPS (`LpipsAlex`, `lpips_video`) restates the reference's lpips.LPIPS(net="alex") on the same 8-bit frames in fp32: AlexNet's five
conv layers as fp32-MFMA implicit GEMMs, the first one reading the videos themselves.  Its weights are USER-SUPPLIED (a torchvision
AlexNet state dict plus the LPIPS linear file, or one full LPIPS state dict); none ship with the package, and without them nothing
changes: result files carry an `LPIPS` line only when LPIPS values were added.  `LpipsAlex.synthetic` gives deterministic weights for
tests and timing, whose scores are not comparable with published LPIPS.  Parity rests on this restatement (tests/lpips_ref.py):
neither torchvision nor the `lpips` package is part of this environment.
Temporal spectra (`temporal_spectrum`, `spectrum_report`; csrc/hv_spectrum.hip) restate the fork's theory_analysis.ipynb: the mean
|FFT| over all pixel time series of the gray frames and over all latent series, as one fp32-MFMA DFT whose product never leaves the chip.
FVD (`I3D`, `fvd_logits`, `frechet_distance`; csrc/hv_i3d.hip) is the `method='videogpt'` path of the fork's calculate_fvd: Inception-I3D
logits of every input clip and every reconstruction as fp32-MFMA 3-D convolutions, then the Frechet distance on the host.  Its weights are
user-supplied too.  The value is "FVD (videogpt I3D logits)", not interchangeable with the styleganv variant (a TorchScript archive).
Gaussian-window SSIM (`gaussian_ssim`, `gaussian_ssim_sums`; csrc/hv_gssim.hip) is the SSIM of the fork's rebuttal tables: an 11-tap
Gaussian over T, H and W (run.py, pytorch_msssim) and per frame (calculate_ssim.py, cv2), in fp64 on the same 8-bit frames.
Content statistics (`content_histograms`, `content_entropy`, `content_bucket`; csrc/hv_content.hip) give the measure behind the fork's
InterEntropy bucket lists - the entropy of the gray frame-difference histogram, a definition of this project's own.
Motion fields (`block_motion`, `motion_stats`, `motion_compare`; csrc/hv_motion.hip) say how much a clip moves and whether its
reconstruction moves the same way: full-search block matching on the gray frames, this project's own measure too, not FVMD.
What it is not: there is no video codec in between (the reference's frames went through libx264).  CPU tensors are refused like
everywhere else in the package."""
from __future__ import annotations

import math
import os
from datetime import datetime

import numpy as np
import torch

from . import _abi, _lib

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


def video_metrics(ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True, lpips: "LpipsAlex" = None, gssim: bool = False) -> dict:
    """PSNR / SSIM per frame of `rec` against `ref` ([C,T,H,W] or [B,C,T,H,W] GPU tensors, fp16 or fp32, values in [-1, 1] with
    rescale=True, [0, 1] without).  One host synchronisation.  Returns float64 numpy arrays `psnr`, `ssim` ([T], or [B,T] for a batch),
    their means `psnr_mean`, `ssim_mean`, and the raw integers `sse`, `minmax` the scores were formed from.  With `lpips` (an
    LpipsAlex) also `lpips` (per frame) and `lpips_mean`; with `gssim` also the keys of gaussian_ssim (`ssim3d`, `ssim2d`, `ssim2d_frames`,
    `temporal`)."""
    batched = ref.dim() == 5
    st = video_stats(ref, rec, rescale)
    B, C, T, H, W = st["shape"]
    if lpips is not None:
        st["lpips_sums"], lp_pixels = _lpips_enqueue(ref, rec, lpips, rescale, None)
    if gssim:
        st["gssim3"], g_temporal, st["gssim2"] = _gssim_enqueue(ref, rec, rescale)
    host = {}
    for k in ("sse", "minmax", "ssim_sum") + (("lpips_sums",) if lpips is not None else ()) + (("gssim3", "gssim2") if gssim else ()):
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
    out = {"psnr": psnr, "ssim": ssim, "psnr_mean": float(psnr.mean()), "ssim_mean": float(ssim.mean()),
           "sse": sse, "minmax": minmax, "ssim_sum": ssim_sum}
    if lpips is not None:
        lp = lpips_from_sums(host["lpips_sums"].numpy(), lp_pixels)[0]
        out["lpips"] = lp if batched else lp[0]
        out["lpips_mean"] = float(lp.mean())
    if gssim:
        g = gssim_from_sums(host["gssim3"].numpy(), host["gssim2"].numpy(), H, W)
        if not batched:
            g = {"ssim3d": float(g["ssim3d"][0]), "ssim2d": float(g["ssim2d"][0]), "ssim2d_frames": g["ssim2d_frames"][0]}
        out.update(g, temporal=g_temporal)
    return out


# ---- Gaussian-window SSIM (csrc/hv_gssim.hip, include/hv_gssim.h) -----------------------------------------------------------------------
# The fork's second scoring programme, rebuttal/common_metrics_on_video_quality: run.py:61-68 calls pytorch_msssim.ssim on the 5-D tensor
# [B,C,T,H,W] (data_range 1: an 11-tap Gaussian, sigma 1.5, over T, H and W, valid positions, C1 = 0.01^2, C2 = 0.03^2) - `ssim3d`;
# calculate_ssim.py beside it applies cv2.getGaussianKernel(11, 1.5) per frame and channel in float64 - `ssim2d`.  Neither package is part
# of this environment: the definition is pinned to this project's restatement (tests/gssim_ref.py).
GSSIM_WIN = _abi.GSSIM_MACROS["HV_GSSIM_WIN"]
GSSIM_SIGMA = 1.5


def gaussian_window(dtype=torch.float32) -> np.ndarray:
    """The 11 weights exp(-(i - 5)^2 / (2 * 1.5^2)) / sum as float64 numpy.  torch.float32: computed and normalised in fp32, then widened
    (pytorch_msssim._fspecial_gauss_1d); torch.float64: the same formula in double (cv2.getGaussianKernel(11, 1.5))."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"gaussian_window: torch.float32 or torch.float64, got {dtype}")
    c = torch.arange(GSSIM_WIN, dtype=dtype) - GSSIM_WIN // 2
    g = torch.exp(-(c ** 2) / (2 * GSSIM_SIGMA ** 2))
    return (g / g.sum()).double().numpy()


_gssim_windows = {}


def _gssim_window_on(device, dtype) -> torch.Tensor:
    key = (str(device), dtype)
    if key not in _gssim_windows:
        _gssim_windows[key] = torch.from_numpy(gaussian_window(dtype)).to(device)
    return _gssim_windows[key]


def gaussian_ssim_sums(ref: torch.Tensor, rec: torch.Tensor, temporal: bool = True, rescale: bool = True, win: torch.Tensor = None):
    """Sums of the Gaussian-window SSIM map, left on the device: float64 [B,To,C], To = T - 10 with `temporal` (the window runs along T, H
    and W) and T without (H and W only); each entry is the sum over the (H - 10) * (W - 10) positions of that output frame and channel.
    [C,T,H,W] inputs count as B = 1; the first min(T_ref, T_rec) frames are scored, as by video_stats.  `win`: 11 float64 weights on the
    device (default: the fp32-form window with `temporal`, the fp64-form one without).  Nothing is synchronised."""
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
    temporal = 1 if temporal else 0
    if win is None:
        win = _gssim_window_on(dev, torch.float32 if temporal else torch.float64)
    if not isinstance(win, torch.Tensor) or win.device != dev or win.dtype != torch.float64 or win.shape != (GSSIM_WIN,) or \
            not win.is_contiguous():
        raise _lib.HVKernelError(f"win: expected {GSSIM_WIN} contiguous float64 weights on {dev}")
    ws_bytes = _lib.host("gaussian_ssim_workspace_bytes", C, T, H, W, temporal)
    if ws_bytes <= 0:
        raise _lib.HVKernelError(f"gaussian_ssim: shape C={C} T={T} H={H} W={W} temporal={temporal} is refused (C 1 | 3, H and W >= "
                                 f"{GSSIM_WIN}, T >= {GSSIM_WIN} with the temporal window)")
    To = T - (GSSIM_WIN - 1) * temporal
    sums = torch.empty(B, To, C, dtype=torch.float64, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    for b in range(B):
        a, r = ref[b], rec[b]
        _lib.call("gaussian_ssim", a, a.stride(0), a.stride(1), a.stride(2), r, r.stride(0), r.stride(1), r.stride(2),
                  _DTYPES[ref.dtype], C, T, H, W, 1 if rescale else 0, temporal, win, sums[b], ws, ws.numel())
    return sums


def _gssim_enqueue(ref, rec, rescale):
    """-> (sums of the run.py score, whether its window spans T, sums of the calculate_ssim.py score), on the device"""
    T = min(ref.shape[-3], rec.shape[-3])
    temporal = T >= GSSIM_WIN
    if not temporal:
        import warnings
        warnings.warn(f"gaussian_ssim: {T} frames are fewer than the window's {GSSIM_WIN}: ssim3d skips the T axis (pytorch_msssim "
                      "does the same), so it is a 2-D score under the fp32-form window", stacklevel=3)
    dev = ref.device
    s3 = gaussian_ssim_sums(ref, rec, temporal, rescale, _gssim_window_on(dev, torch.float32))
    s2 = gaussian_ssim_sums(ref, rec, False, rescale, _gssim_window_on(dev, torch.float64))
    return s3, temporal, s2


def gssim_from_sums(sums3d, sums2d, H: int, W: int) -> dict:
    """host rules on the sums [B,To,C] and [B,T,C] (numpy float64): ssim3d [B] = mean over channels, output frames and positions (run.py);
    ssim2d_frames [B,T] = per frame the mean over channels, ssim2d [B] = their mean over frames (calculate_ssim.py)"""
    npos = float((H - GSSIM_WIN + 1) * (W - GSSIM_WIN + 1))
    s3, s2 = np.asarray(sums3d, dtype=np.float64), np.asarray(sums2d, dtype=np.float64)
    frames = (s2 / npos).mean(axis=2)
    return {"ssim3d": (s3 / npos).mean(axis=(1, 2)), "ssim2d": frames.mean(axis=1), "ssim2d_frames": frames}


def gaussian_ssim(ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True) -> dict:
    """Both Gaussian-window scores of `rec` against `ref` ([C,T,H,W] or [B,C,T,H,W] GPU tensors as video_metrics takes them); one host
    synchronisation.  `ssim3d`: the run.py score (fp32-form window over T, H, W; with fewer than 11 frames over H, W only, with a
    warning); `ssim2d`: the calculate_ssim.py score (fp64-form window per frame); `ssim2d_frames`: its per-frame values; `temporal`:
    whether ssim3d's window spanned T.  Floats and [T] for one video, [B] and [B,T] for a batch."""
    batched = ref.dim() == 5
    s3, temporal, s2 = _gssim_enqueue(ref, rec, rescale)
    h3 = torch.empty(s3.shape, dtype=s3.dtype, pin_memory=True).copy_(s3, non_blocking=True)
    h2 = torch.empty(s2.shape, dtype=s2.dtype, pin_memory=True).copy_(s2, non_blocking=True)
    torch.cuda.current_stream(ref.device).synchronize()
    out = gssim_from_sums(h3.numpy(), h2.numpy(), ref.shape[-2], ref.shape[-1])
    if not batched:
        out = {"ssim3d": float(out["ssim3d"][0]), "ssim2d": float(out["ssim2d"][0]), "ssim2d_frames": out["ssim2d_frames"][0]}
    out["temporal"] = temporal
    return out


# ---- LPIPS (AlexNet) ------------------------------------------------------------------------------------------------------------------
# torchvision alexnet features[0:12] as lpips/pretrained_networks.py:56-94 slices it: (features index, Cin, Cout, kernel, stride, pad);
# a maxpool 3/2 follows taps 1 and 2, the trailing one is unused
LPIPS_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
LPIPS_CHNS = tuple(c[2] for c in LPIPS_CONVS)
LPIPS_MIN_SIZE = 31          # the smallest input whose tap 3-5 maps are 1 x 1
_LPIPS_CHUNK_BYTES = 1 << 29   # default bound of the two feature buffers together


def lpips_lut() -> torch.Tensor:
    """float32 [3, 256]: the network input of 8-bit value q in channel c, with exactly the reference's operations -
    compute_metrics.py:44-60 `torch.from_numpy(img / 255.0).float() * 2 - 1` (the division in float64, the rest in fp32), then the
    ScalingLayer `(x - shift) / scale` (lpips.py:147-154)."""
    q = torch.arange(256, dtype=torch.float64)
    x = (q / 255.0).float() * 2 - 1
    shift = torch.Tensor([-.030, -.088, -.188])[:, None]
    scale = torch.Tensor([.458, .448, .450])[:, None]
    return (x[None, :] - shift) / scale


def lpips_map_sizes(H: int, W: int):
    """[(h, w)] of the five taps for an H x W input"""
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


def lpips_buffer_plan(H: int, W: int):
    """-> (pixels of the five taps, floats per image of a ping-pong feature buffer - the largest of the taps and the two pooled maps,
    default frames per chunk: as many as keep the two buffers, 2 images per frame each, within _LPIPS_CHUNK_BYTES)"""
    pixels = [h * w for h, w in lpips_map_sizes(H, W)]
    per_image = max(max(p * c for p, c in zip(pixels, LPIPS_CHNS)), pixels[1] * LPIPS_CHNS[0], pixels[2] * LPIPS_CHNS[1])
    return pixels, per_image, max(1, _LPIPS_CHUNK_BYTES // (2 * 2 * per_image * 4))


def lpips_pack_conv(w: torch.Tensor, first: bool) -> torch.Tensor:
    """torch [Cout, Cin, k, k] -> the kernels' k-major [Kpad, Cout]: first layer k = (c * 11 + ky) * 11 + kx with zero rows up to 384,
    the others k = (ky * ksize + kx) * Cin + ci"""
    co = w.shape[0]
    if first:
        out = torch.zeros(384, co, dtype=torch.float32)
        out[:363] = w.reshape(co, 363).T
        return out
    return w.permute(2, 3, 1, 0).reshape(-1, co).contiguous()


class LpipsAlex:
    """Weights of lpips.LPIPS(net="alex", version="0.1"): five conv layers (torch layout, fp32) and five non-negative `lin` vectors.
    Built on the host; the packed device copies are made on first use per device."""

    def __init__(self, convs, lins, label: str = "user"):
        if len(convs) != 5 or len(lins) != 5:
            raise ValueError("LpipsAlex needs 5 conv layers and 5 lin vectors")
        self.convs, self.lins, self.label = [], [], label
        for i, ((w, b), lin, (_, ci, co, k, _, _)) in enumerate(zip(convs, lins, LPIPS_CONVS)):
            w, b, lin = w.detach().float().cpu(), b.detach().float().cpu(), lin.detach().float().cpu().reshape(-1)
            if tuple(w.shape) != (co, ci, k, k) or tuple(b.shape) != (co,) or lin.numel() != co:
                raise ValueError(f"LPIPS layer {i + 1}: expected weight {(co, ci, k, k)}, bias {(co,)}, lin {co} values; got "
                                 f"{tuple(w.shape)}, {tuple(b.shape)}, {lin.numel()}")
            self.convs.append((w.contiguous(), b.contiguous()))
            self.lins.append(lin.contiguous())
        self._dev = {}

    @classmethod
    def from_state_dict(cls, sd: dict, linear_sd: dict = None, label: str = "user") -> "LpipsAlex":
        """`sd`: a torchvision AlexNet state dict (features.{0,3,6,8,10}.{weight,bias}; other keys ignored) with the LPIPS linear
        layers in `linear_sd` (lin{0..4}.model.1.weight, [1,C,1,1]) - or one full LPIPS state dict (net.slice{1..5}.{0,3,6,8,10}.* and
        lin*) on its own."""
        merged = dict(sd)
        if linear_sd is not None:
            merged.update(linear_sd)
        convs, lins, missing = [], [], []
        for i, (idx, *_rest) in enumerate(LPIPS_CONVS):
            names = [(f"features.{idx}.weight", f"features.{idx}.bias"), (f"net.slice{i + 1}.{idx}.weight", f"net.slice{i + 1}.{idx}.bias")]
            got = [n for n in names if n[0] in merged and n[1] in merged]
            if got:
                convs.append((merged[got[0][0]], merged[got[0][1]]))
            else:
                missing.append(f"features.{idx}.{{weight,bias}} (or net.slice{i + 1}.{idx}.*)")
            if f"lin{i}.model.1.weight" in merged:
                lins.append(merged[f"lin{i}.model.1.weight"])
            else:
                missing.append(f"lin{i}.model.1.weight")
        if missing:
            raise ValueError("LPIPS weights are incomplete, missing: " + ", ".join(missing))
        return cls(convs, lins, label)

    @classmethod
    def from_files(cls, alexnet_path, linear_path=None) -> "LpipsAlex":
        """Tensor files read without executing anything from them (checkpoint.read_tensors: .pt / .pth with weights_only, .safetensors)."""
        from .checkpoint import read_tensors
        return cls.from_state_dict(read_tensors(alexnet_path), read_tensors(linear_path) if linear_path else None)

    @classmethod
    def synthetic(cls, seed: int = 0) -> "LpipsAlex":
        """Deterministic stand-in weights: conv hashed_uniform * sqrt(6 / fan_in), bias 0.1 * hashed_uniform, lin 0.5 * |hashed_uniform|.
        Scores under them are NOT comparable with published LPIPS."""
        from .synthetic import hashed_uniform
        convs, lins = [], []
        for i, (_, ci, co, k, _, _) in enumerate(LPIPS_CONVS):
            convs.append((hashed_uniform((co, ci, k, k), f"lpips.conv{i}.weight", seed) * math.sqrt(6.0 / (ci * k * k)),
                          0.1 * hashed_uniform((co,), f"lpips.conv{i}.bias", seed)))
            lins.append(0.5 * hashed_uniform((co,), f"lpips.lin{i}", seed).abs())
        return cls(convs, lins, label="synthetic")

    def on(self, device) -> dict:
        """{"w": [5 packed], "b": [5], "lin": [5], "lut": [3,256]} on `device`"""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = {"w": [lpips_pack_conv(w, i == 0).to(device) for i, (w, _) in enumerate(self.convs)],
                                 "b": [b.to(device) for _, b in self.convs], "lin": [v.to(device) for v in self.lins],
                                 "lut": lpips_lut().contiguous().to(device)}
        return self._dev[device]


def _lpips_chunk(a, r, wts, rescale, Tc, H, W, bufs, ws, out):
    """the launches of frames [0, Tc) of one video pair; out [Tc, 5] float64 layer sums"""
    N = 2 * Tc
    sizes = lpips_map_sizes(H, W)
    src, dst = bufs

    def dist(layer, f):
        h, w = sizes[layer]
        _lib.call("lpips_distance_f32", f, wts["lin"][layer], Tc, h * w, LPIPS_CHNS[layer], layer, out, ws, ws.numel())

    _lib.call("lpips_conv1_f32", a, a.stride(0), a.stride(1), a.stride(2), r, r.stride(0), r.stride(1), r.stride(2), _DTYPES[a.dtype],
              Tc, H, W, 1 if rescale else 0, wts["lut"], wts["w"][0], wts["b"][0], src)
    dist(0, src)
    for layer in range(1, 5):
        _, ci, co, k, _, pad = LPIPS_CONVS[layer]
        h, w = sizes[layer]
        if layer <= 2:                        # taps 1 and 2 are pooled before the next conv
            ph, pw = sizes[layer - 1]
            _lib.call("lpips_maxpool_f32", src, dst, N, ph, pw, ci)
            src, dst = dst, src
        _lib.call("lpips_conv2d_f32", src, wts["w"][layer], wts["b"][layer], dst, N, h, w, ci, co, k, pad)
        src, dst = dst, src
        dist(layer, src)


def _lpips_enqueue(ref, rec, model, rescale, frames_per_chunk):
    """-> (device float64 [B, T, 5] layer sums, pixel counts of the five taps); nothing is synchronised"""
    if not isinstance(model, LpipsAlex):
        raise TypeError(f"lpips: expected an LpipsAlex, got {type(model).__name__}")
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
    if C != 3:
        raise _lib.HVKernelError(f"LPIPS reads RGB videos, got C = {C}")
    if H < LPIPS_MIN_SIZE or W < LPIPS_MIN_SIZE:
        raise _lib.HVKernelError(f"LPIPS (AlexNet) needs H, W >= {LPIPS_MIN_SIZE}, got {H} x {W}")
    T = min(ref.shape[2], rec.shape[2])
    dev = ref.device
    pixels, per_image, default_chunk = lpips_buffer_plan(H, W)
    Tc = max(1, min(T, int(default_chunk if frames_per_chunk is None else frames_per_chunk)))
    wts = model.on(dev)
    bufs = [torch.empty(2 * Tc * per_image, dtype=torch.float32, device=dev) for _ in range(2)]
    ws = torch.empty(max(_lib.host("lpips_distance_workspace_bytes", Tc, pixels[0]), 16), dtype=torch.uint8, device=dev)
    out = torch.empty(B, T, 5, dtype=torch.float64, device=dev)
    for b in range(B):                        # one stream: each launch reuses the buffers after the launches before it
        for t0 in range(0, T, Tc):
            n = min(Tc, T - t0)
            _lpips_chunk(ref[b][:, t0:t0 + n], rec[b][:, t0:t0 + n], wts, rescale, n, H, W, bufs, ws, out[b, t0:t0 + n])
    return out, pixels


def lpips_from_sums(sums, pixels):
    """layer sums [..., 5] (numpy float64) -> (LPIPS [...], per-layer values [..., 5]): spatial_average and the sum over taps
    (lpips.py:130,137-139)"""
    layers = np.asarray(sums, dtype=np.float64) / np.asarray(pixels, dtype=np.float64)
    return layers.sum(axis=-1), layers


def lpips_video(ref: torch.Tensor, rec: torch.Tensor, model: LpipsAlex, rescale: bool = True, frames_per_chunk: int = None,
                return_layers: bool = False):
    """LPIPS (AlexNet) per frame of `rec` against `ref`, under the input rules of `video_stats` (GPU only, fp16 / fp32, C = 3, the
    first min(T_ref, T_rec) frames, W contiguous, strided views allowed; H, W >= 31).  Frames go through the network `frames_per_chunk`
    at a time (default: as many as keep the two feature buffers within 512 MiB), all on the current stream, with one host
    synchronisation at the end; a frame's value does not depend on the chunking.  Returns float64 [T] ([B,T] for a batch); with
    return_layers also the per-tap values [T,5]."""
    batched = ref.dim() == 5 if isinstance(ref, torch.Tensor) else False
    sums, pixels = _lpips_enqueue(ref, rec, model, rescale, frames_per_chunk)
    host = torch.empty(sums.shape, dtype=sums.dtype, pin_memory=True)
    host.copy_(sums, non_blocking=True)
    torch.cuda.current_stream(sums.device).synchronize()
    total, layers = lpips_from_sums(host.numpy().copy(), pixels)
    if not batched:
        total, layers = total[0], layers[0]
    return (total, layers) if return_layers else total


# ---- FVD: Inception-I3D logits (csrc/hv_i3d.hip) and the Frechet distance -----------------------------------------------------------------
# The fork's rebuttal/common_metrics_on_video_quality/calculate_fvd.py with method='videogpt': fvd/videogpt/pytorch_i3d.py is the network,
# fvd/videogpt/fvd.py the preprocessing and the distance.  The number is "FVD (videogpt I3D logits)": it is NOT interchangeable with the
# styleganv variant (a TorchScript detector, pickled code this package does not load), which is the default of the fork's run.py.
FVD_LABEL = "FVD (videogpt I3D logits)"
FVD_NOTE = "not interchangeable with the styleganv variant"
I3D_CLASSES = 400
I3D_MIN_FRAMES = 10          # calculate_fvd.py:33 asserts it
I3D_SIZE = 224
I3D_MIN_SIDE = 193           # the smallest side whose five halvings end at 7, what the head's 7 x 7 average pool needs
I3D_BN_EPS = 1e-5

# Inception modules (pytorch_i3d.py:229-272): name, Cin, (b0, b1a, b1b, b2a, b2b, b3b) output channels
I3D_MIXED = (("Mixed_3b", 192, (64, 96, 128, 16, 32, 32)), ("Mixed_3c", 256, (128, 128, 192, 32, 96, 64)),
             ("Mixed_4b", 480, (192, 96, 208, 16, 48, 64)), ("Mixed_4c", 512, (160, 112, 224, 24, 64, 64)),
             ("Mixed_4d", 512, (128, 128, 256, 24, 64, 64)), ("Mixed_4e", 512, (112, 144, 288, 32, 64, 64)),
             ("Mixed_4f", 528, (256, 160, 320, 32, 128, 128)), ("Mixed_5b", 832, (256, 160, 320, 32, 128, 128)),
             ("Mixed_5c", 832, (384, 192, 384, 48, 128, 128)))
_I3D_POOL_BEFORE = {"Mixed_4b": ("MaxPool3d_4a_3x3", (3, 3, 3), (2, 2, 2)), "Mixed_5b": ("MaxPool3d_5a_2x2", (2, 2, 2), (2, 2, 2))}


def _i3d_layer_table():
    """The network as one flat table, in launch order: (name, kind, Cin, Cout, kernel, stride, source, destination), kind "conv" | "pool"
    | "head", source / destination = (buffer, first column, row pitch).  Buffers 0 and 1 alternate as the current feature map, 2 is an
    Inception module's scratch ([b1a | b2a | pooled input] side by side), -1 the 4-channel input, -2 the logits.  A conv's name is its
    state-dict prefix."""
    rows = []
    one, three = (1, 1, 1), (3, 3, 3)
    rows.append(("Conv3d_1a_7x7", "conv", 4, 64, (7, 7, 7), (2, 2, 2), (-1, 0, 4), (0, 0, 64)))
    rows.append(("MaxPool3d_2a_3x3", "pool", 64, 64, (1, 3, 3), (1, 2, 2), (0, 0, 64), (1, 0, 64)))
    rows.append(("Conv3d_2b_1x1", "conv", 64, 64, one, one, (1, 0, 64), (0, 0, 64)))
    rows.append(("Conv3d_2c_3x3", "conv", 64, 192, three, one, (0, 0, 64), (1, 0, 192)))
    rows.append(("MaxPool3d_3a_3x3", "pool", 192, 192, (1, 3, 3), (1, 2, 2), (1, 0, 192), (0, 0, 192)))
    cur, width = 0, 192
    for name, cin, (o0, o1, o2, o3, o4, o5) in I3D_MIXED:
        assert cin == width, name
        if name in _I3D_POOL_BEFORE:
            pname, k, s = _I3D_POOL_BEFORE[name]
            rows.append((pname, "pool", cin, cin, k, s, (cur, 0, cin), (1 - cur, 0, cin)))
            cur = 1 - cur
        out, cout, sp = 1 - cur, o0 + o2 + o4 + o5, o1 + o3 + cin
        src = (cur, 0, cin)
        rows.append((f"{name}.b0", "conv", cin, o0, one, one, src, (out, 0, cout)))
        rows.append((f"{name}.b1a", "conv", cin, o1, one, one, src, (2, 0, sp)))
        rows.append((f"{name}.b1b", "conv", o1, o2, three, one, (2, 0, sp), (out, o0, cout)))
        rows.append((f"{name}.b2a", "conv", cin, o3, one, one, src, (2, o1, sp)))
        rows.append((f"{name}.b2b", "conv", o3, o4, three, one, (2, o1, sp), (out, o0 + o2, cout)))
        rows.append((f"{name}.b3a", "pool", cin, cin, three, one, src, (2, o1 + o3, sp)))
        rows.append((f"{name}.b3b", "conv", cin, o5, one, one, (2, o1 + o3, sp), (out, o0 + o2 + o4, cout)))
        cur, width = out, cout
    rows.append(("logits", "head", width, I3D_CLASSES, (2, 7, 7), one, (cur, 0, width), (-2, 0, I3D_CLASSES)))
    return tuple(rows)


I3D_LAYERS = _i3d_layer_table()
I3D_CONVS = tuple((r[0], 3 if r[0] == "Conv3d_1a_7x7" else r[2], r[3], r[4]) for r in I3D_LAYERS if r[1] == "conv")   # state-dict shapes


def i3d_same_pad(k: int, s: int, extent: int):
    """The TF-"same" rule of pytorch_i3d.py:9-30,71-93 for one axis -> (cells of zero padding in front, output extent): the total is
    max(k - s, 0) if extent % s == 0 else max(k - extent % s, 0), the front gets total // 2, the output is ceil(extent / s)."""
    total = max(k - s, 0) if extent % s == 0 else max(k - extent % s, 0)
    return total // 2, -(-extent // s)


def i3d_walk(T: int, H: int, W: int):
    """I3D_LAYERS with extents: yields (row, input extents (T, H, W), output extents, front pads) per layer"""
    ext = {-1: (T, H, W)}
    for row in I3D_LAYERS:
        _, kind, _, _, k, s, src, dst = row
        e = ext[src[0]]
        if kind == "head":
            yield row, e, (1, 1, 1), (0, 0, 0)
            continue
        pads, out = zip(*(i3d_same_pad(k[a], s[a], e[a]) for a in range(3)))
        ext[dst[0]] = tuple(out)
        yield row, e, tuple(out), tuple(pads)


def i3d_buffer_plan(T: int, H: int, W: int) -> dict:
    """Floats of the three feature buffers a [T,H,W,4] input needs (each reused across layers: the largest voxels x pitch it ever holds),
    the frames T' of the last map, and the peak in bytes - input, buffers and the head's workspace together."""
    floats = [0, 0, 0]
    head_t = None
    for (name, kind, _, _, _, _, src, dst), e, o, _ in i3d_walk(T, H, W):
        if kind == "head":
            head_t = e[0]
            if e[1] != 7 or e[2] != 7 or e[0] < 2:
                raise _lib.HVKernelError(f"I3D: a {T} x {H} x {W} input ends in a {e[0]} x {e[1]} x {e[2]} map; the head needs T' >= 2 and "
                                         f"7 x 7 (T >= 9 frames, {I3D_MIN_SIDE} <= H, W <= {I3D_SIZE})")
            continue
        floats[dst[0]] = max(floats[dst[0]], o[0] * o[1] * o[2] * dst[2])
    ws = (head_t - 1) * 1024
    return {"floats": floats, "head_frames": head_t, "workspace_floats": ws,
            "peak_bytes": 4 * (T * H * W * 4 + sum(floats) + ws + I3D_CLASSES)}


def i3d_pack_conv(w: torch.Tensor) -> torch.Tensor:
    """torch [Cout, Cin, kt, kh, kw] -> the kernel's k-major [Kpad, Cout], k = ((dt * kh + dh) * kw + dw) * Cin + ci; a 3-channel input
    layer gets a zero fourth channel, K is rounded up to 32 with zero rows"""
    co, ci = w.shape[:2]
    if ci % 4:
        w = torch.cat([w, torch.zeros(co, 4 - ci % 4, *w.shape[2:], dtype=w.dtype)], dim=1)
    k = w.permute(2, 3, 4, 1, 0).reshape(-1, co)
    out = torch.zeros(-(-k.shape[0] // 32) * 32, co, dtype=torch.float32)
    out[:k.shape[0]] = k
    return out


def i3d_fold_bn(gamma, beta, mean, var, eps: float = I3D_BN_EPS):
    """eval-mode BatchNorm3d as y = x * sc + sh: sc = gamma / sqrt(var + eps), sh = beta - mean * sc, in fp64, each rounded to fp32 once"""
    g, b, m, v = (t.detach().double().cpu() for t in (gamma, beta, mean, var))
    sc = g / torch.sqrt(v + eps)
    return sc.float(), (b - m * sc).float()


class I3D:
    """Weights of the reference's InceptionI3d(400, in_channels=3) in eval mode, under its state-dict names (`Conv3d_1a_7x7.conv3d.weight`,
    `Mixed_4b.b1b.bn.running_var`, `logits.conv3d.bias`, ...).  USER-SUPPLIED (i3d_pretrained_400.pt is a plain state dict); none ship
    with the package.  Built on the host; the BatchNorm fold and the packed device copies are made once per device."""

    def __init__(self, sd: dict, label: str = "user"):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        self.sd, self.label = {}, label

        def take(key, shape):
            if key not in sd:
                raise ValueError(f"I3D weights: missing key {key!r}")
            t = sd[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
                raise ValueError(f"I3D weights: {key!r} must be a tensor of shape {tuple(shape)}, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            self.sd[key] = t.detach().float().cpu().contiguous()

        for name, ci, co, k in I3D_CONVS:
            take(f"{name}.conv3d.weight", (co, ci, *k))
            for p in ("weight", "bias", "running_mean", "running_var"):
                take(f"{name}.bn.{p}", (co,))
        take("logits.conv3d.weight", (I3D_CLASSES, 1024, 1, 1, 1))
        take("logits.conv3d.bias", (I3D_CLASSES,))
        self._dev = {}

    @classmethod
    def from_state_dict(cls, sd: dict, label: str = "user") -> "I3D":
        return cls(sd, label)

    @classmethod
    def from_file(cls, path) -> "I3D":
        """A tensor file read without executing anything from it (checkpoint.read_tensors: .pt / .pth with weights_only, .safetensors)."""
        from .checkpoint import read_tensors
        return cls(read_tensors(path))

    @classmethod
    def synthetic(cls, seed: int = 0) -> "I3D":
        """Deterministic stand-in weights: conv hashed_uniform * sqrt(6 / fan_in) (He), BatchNorm gamma in [0.8, 1.2], beta and running
        mean in [-0.1, 0.1], running variance in [0.5, 1.5], logits bias in [-0.1, 0.1].  About half of every layer's units stay live.
        Distances under them are NOT comparable with published FVD."""
        from .synthetic import hashed_uniform as hu
        sd = {}
        for name, ci, co, k in I3D_CONVS:
            sd[f"{name}.conv3d.weight"] = hu((co, ci, *k), f"i3d.{name}.weight", seed) * math.sqrt(6.0 / (ci * k[0] * k[1] * k[2]))
            sd[f"{name}.bn.weight"] = 1.0 + 0.2 * hu((co,), f"i3d.{name}.gamma", seed)
            sd[f"{name}.bn.bias"] = 0.1 * hu((co,), f"i3d.{name}.beta", seed)
            sd[f"{name}.bn.running_mean"] = 0.1 * hu((co,), f"i3d.{name}.mean", seed)
            sd[f"{name}.bn.running_var"] = 1.0 + 0.5 * hu((co,), f"i3d.{name}.var", seed)
        sd["logits.conv3d.weight"] = hu((I3D_CLASSES, 1024, 1, 1, 1), "i3d.logits.weight", seed) * math.sqrt(6.0 / 1024)
        sd["logits.conv3d.bias"] = 0.1 * hu((I3D_CLASSES,), "i3d.logits.bias", seed)
        return cls(sd, label="synthetic")

    def state_dict(self) -> dict:
        """the tensors under the reference's key names (fp32, host)"""
        return dict(self.sd)

    def folded(self, name: str):
        """(sc, sh) fp32 of conv `name`: its BatchNorm folded"""
        return i3d_fold_bn(*(self.sd[f"{name}.bn.{p}"] for p in ("weight", "bias", "running_mean", "running_var")))

    def on(self, device) -> dict:
        """{conv name: (packed w, sc, sh)} and "logits": (w [1024, 400], bias) on `device`"""
        device = torch.device(device)
        if device not in self._dev:
            d = {}
            for name, _, _, _ in I3D_CONVS:
                sc, sh = self.folded(name)
                d[name] = (i3d_pack_conv(self.sd[f"{name}.conv3d.weight"]).to(device), sc.to(device), sh.to(device))
            d["logits"] = (self.sd["logits.conv3d.weight"].reshape(I3D_CLASSES, 1024).T.contiguous().to(device),
                           self.sd["logits.conv3d.bias"].to(device))
            self._dev[device] = d
        return self._dev[device]


def _i3d_buffers(plan, dev):
    return ([torch.empty(max(n, 4), dtype=torch.float32, device=dev) for n in plan["floats"]],
            torch.empty(plan["workspace_floats"], dtype=torch.float32, device=dev))


def _i3d_enqueue(x_cl, wts, bufs, ws, out):
    """the launches of one clip: x_cl [T,H,W,4] fp32 contiguous -> out [400]"""
    T, H, W, _ = x_cl.shape
    flat = {-1: x_cl.reshape(-1), -2: out, 0: bufs[0], 1: bufs[1], 2: bufs[2]}
    for (name, kind, ci, co, k, s, src, dst), e, _, pads in i3d_walk(T, H, W):
        x, y = flat[src[0]][src[1]:], flat[dst[0]][dst[1]:]
        if kind == "conv":
            w, sc, sh = wts[name]
            _lib.call("i3d_conv3d_f32", x, src[2], w, sc, sh, y, dst[2], e[0], e[1], e[2], ci, co, *k, *s, *pads, 1)
        elif kind == "pool":
            _lib.call("i3d_maxpool3d_f32", x, src[2], y, dst[2], e[0], e[1], e[2], ci, *k, *s, *pads)
        else:
            w, b = wts["logits"]
            _lib.call("i3d_head_f32", x, src[2], w, b, y, e[0], e[1], e[2], ci, ws, ws.numel())


def _check_i3d_model(model):
    if not isinstance(model, I3D):
        raise TypeError(f"fvd: expected an I3D, got {type(model).__name__}")


def i3d_logits(x_cl: torch.Tensor, model: I3D) -> torch.Tensor:
    """The network alone: x_cl [T,H,W,4] fp32 on the GPU (channels-last voxels, channel 3 = 0; 193 <= H, W <= 224, T >= 9 so that the
    last map is T' >= 2 frames of 7 x 7) -> float32 [400] on the device.  Nothing is synchronised."""
    _check_i3d_model(model)
    if not isinstance(x_cl, torch.Tensor) or not x_cl.is_cuda:
        raise _lib.HVKernelError("i3d_logits: expected a GPU tensor (this package has no CPU path)")
    if x_cl.dtype != torch.float32 or x_cl.dim() != 4 or x_cl.shape[-1] != 4 or not x_cl.is_contiguous():
        raise _lib.HVKernelError(f"i3d_logits: expected a contiguous fp32 [T,H,W,4] tensor, got {x_cl.dtype} {tuple(x_cl.shape)}")
    T, H, W, _ = x_cl.shape
    plan = i3d_buffer_plan(T, H, W)
    bufs, ws = _i3d_buffers(plan, x_cl.device)
    out = torch.empty(I3D_CLASSES, dtype=torch.float32, device=x_cl.device)
    _i3d_enqueue(x_cl, model.on(x_cl.device), bufs, ws, out)
    return out


def i3d_resized(H: int, W: int):
    """(RH, RW) of fvd.py:32-36 in its own double arithmetic: the shorter side goes to 224, the other to ceil(side * (224 / min(H, W)))"""
    scale = I3D_SIZE / min(H, W)
    return (I3D_SIZE, math.ceil(W * scale)) if H < W else (math.ceil(H * scale), I3D_SIZE)


def fvd_preprocess(video: torch.Tensor, rescale: bool = True) -> torch.Tensor:
    """[3,T,H,W] fp16 / fp32 GPU video (values in [-1, 1] with rescale, [0, 1] without; W contiguous, strided views allowed) -> the
    network input [T,224,224,4] fp32 (fvd.py:21-60 on the 8-bit frames every other score sees; channel 3 = 0)"""
    _check_video(video, "video")
    if video.dim() != 4 or video.shape[0] != 3:
        raise _lib.HVKernelError(f"fvd: expected one RGB clip [3,T,H,W], got {tuple(video.shape)}")
    _, T, H, W = video.shape
    RH, RW = i3d_resized(H, W)
    y = torch.empty(T, I3D_SIZE, I3D_SIZE, 4, dtype=torch.float32, device=video.device)
    _lib.call("i3d_preprocess", video, video.stride(0), video.stride(1), video.stride(2), _DTYPES[video.dtype], T, H, W, RH, RW,
              1 if rescale else 0, y)
    return y


def fvd_logits(video: torch.Tensor, model: I3D, rescale: bool = True) -> torch.Tensor:
    """I3D logits of one clip [3,T,H,W] (or of each clip of a batch [B,3,T,H,W], one after another: clip i of a batch equals its single
    run bit for bit) -> float32 [400] ([B,400]) on the device.  T >= 10, as the reference asserts, else ValueError.  Nothing is
    synchronised."""
    _check_i3d_model(model)
    _check_video(video, "video")
    clips = video[None] if video.dim() == 4 else video
    if clips.shape[1] != 3:
        raise _lib.HVKernelError(f"fvd: expected RGB clips, got C = {clips.shape[1]}")
    T = clips.shape[2]
    if T < I3D_MIN_FRAMES:
        raise ValueError(f"fvd: a clip needs at least {I3D_MIN_FRAMES} frames, got {T}")
    dev = clips.device
    bufs, ws = _i3d_buffers(i3d_buffer_plan(T, I3D_SIZE, I3D_SIZE), dev)
    wts = model.on(dev)
    out = torch.empty(clips.shape[0], I3D_CLASSES, dtype=torch.float32, device=dev)
    for b in range(clips.shape[0]):           # one stream: clip b + 1 reuses the buffers after clip b's launches
        _i3d_enqueue(fvd_preprocess(clips[b], rescale), wts, bufs, ws, out[b])
    return out[0] if video.dim() == 4 else out


def _sym_sqrt(mat: np.ndarray, eps: float = 1e-10) -> np.ndarray:
    """fvd.py:68-71: u diag(s < eps ? s : sqrt(s)) v^T of the SVD"""
    u, s, vt = np.linalg.svd(mat)
    return (u * np.where(s < eps, s, np.sqrt(s))) @ vt


def frechet_distance(f1, f2) -> float:
    """fvd.py:113-125 on the host in fp64: f1 [N1, D], f2 [N2, D] feature sets (numpy or tensors) ->
    tr(S1 + S2) - 2 tr((S1^1/2 S2 S1^1/2)^1/2) + |m1 - m2|^2 with unbiased covariances; the mean term alone for one sample."""
    x1, x2 = (np.asarray(f.detach().cpu().numpy() if isinstance(f, torch.Tensor) else f, dtype=np.float64) for f in (f1, f2))
    x1, x2 = x1.reshape(x1.shape[0], -1), x2.reshape(x2.shape[0], -1)
    if x1.shape[1] != x2.shape[1] or x1.shape[0] < 1 or x2.shape[0] < 1:
        raise ValueError(f"frechet_distance: feature sets {x1.shape} and {x2.shape} do not match")
    m1, m2 = x1.mean(axis=0), x2.mean(axis=0)
    mean = float(((m1 - m2) ** 2).sum())
    if x1.shape[0] == 1:
        return mean
    if x2.shape[0] == 1:
        raise ValueError("frechet_distance: the second set has one sample and the first several: no covariance to compare")
    c1, c2 = ((x - m).T @ (x - m) / (x.shape[0] - 1) for x, m in ((x1, m1), (x2, m2)))
    r1 = _sym_sqrt(c1)
    return float(np.trace(c1 + c2) - 2.0 * np.trace(_sym_sqrt(r1 @ (c2 @ r1))) + mean)


def fvd_caption(clips: int, synthetic: bool = False) -> str:
    """what stands beside every printed and written FVD value: the variant, the clip count (below 400 clips the covariances are
    singular), under stand-in weights the warning"""
    return (f"{FVD_LABEL}, {clips} clips{' < 400: singular covariances' if clips < I3D_CLASSES else ''}; {FVD_NOTE}"
            f"{'; SYNTHETIC I3D weights: not comparable with published FVD' if synthetic else ''}")


def fvd_line(value: float, clips: int, synthetic: bool = False) -> str:
    """the value of a result file's `FVD:` line"""
    return f"{value} [{fvd_caption(clips, synthetic)}]"


def add_fvd_arguments(parser):
    """--fvd-i3d PATH | --fvd-synthetic"""
    parser.add_argument("--fvd-i3d", type=str, default=None, help=f"score {FVD_LABEL} too: the I3D state dict i3d_pretrained_400.pt "
                        f"(.pt / .pth / .safetensors; weights are not shipped); {FVD_NOTE}")
    parser.add_argument("--fvd-synthetic", action="store_true", help="FVD under deterministic synthetic I3D weights: exercises the kernels; "
                        "the value is NOT comparable with published FVD")


def fvd_from_args(args, parser=None, score=True):
    """the I3D the flags of add_fvd_arguments ask for, or None; `score`: whether the driver's --score (where it has one) is set"""
    def fail(msg):
        if parser is not None:
            parser.error(msg)
        raise ValueError(msg)
    path, synthetic = getattr(args, "fvd_i3d", None), bool(getattr(args, "fvd_synthetic", False))
    if (path or synthetic) and not score:
        fail("--fvd-* flags are only valid with --score")
    if path and synthetic:
        fail("--fvd-synthetic and --fvd-i3d exclude each other")
    if synthetic:
        print(f"FVD: synthetic I3D weights - the {FVD_LABEL} value is not comparable with published FVD")
        return I3D.synthetic(0)
    if path:
        return I3D.from_file(path)
    return None


# ---- temporal spectra (csrc/hv_spectrum.hip) --------------------------------------------------------------------------------------------
# The fork's theory_analysis.ipynb, cells 2, 4 and 5: `np.abs(np.fft.fft(signal, axis=0)).mean(axis=1)` over every pixel time series of
# the 8-bit gray frames of a clip (cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY)), and the same over every (channel, h, w) series of
# `latent_dist.mean`, plotted against fftfreq(T, 1 / fps) and fftfreq(T_lat, 4 / fps).
# longest series; frames per k-chunk, bins per column tile (cos block | sin block) of the kernel
SPECTRUM_MAX_T, SPECTRUM_BK, SPECTRUM_BINS = (_abi.MACROS["HV_SPECTRUM_" + k] for k in ("MAX_T", "BK", "BINS"))
# (wr, wg, wb, round, shift) of the integer luma.  UNPINNED RESTATEMENT: OpenCV's 8-bit BGR2GRAY fixed-point rule as far as it can be
# established without cv2 (not part of this environment) - 0.299 / 0.587 / 0.114 in 15 fractional bits, round to nearest.  OpenCV
# builds that take the 14-bit rule (4899, 9617, 1868, 1 << 13, 14) differ by one grey level on a few pixels; pass `luma=` to choose.
GRAY_LUMA = (9798, 19235, 3735, 1 << 14, 15)
_SPECTRUM_MODES = {"gray": 0, "raw": 1}
_twiddle_cache = {}


def spectrum_twiddles(T: int) -> torch.Tensor:
    """The kernel's B operand, float32 [T rounded up to 32, 64 * ncol] on the host: column 64 j + c is cos (c < 32) or sin (c >= 32) of
    2 pi ((k t) mod T) / T for bin k = 1 + 32 j + (c & 31) - the cos and the sin block of the same 32 bins side by side, so that re_k and
    im_k of a series land in one lane.  Every entry is computed in float64 from the integer-reduced k t mod T and rounded once; columns
    of bins behind T // 2 and rows behind T are zero."""
    if not 1 <= T <= SPECTRUM_MAX_T:
        raise _lib.HVKernelError(f"temporal spectrum: 1 <= T <= {SPECTRUM_MAX_T}, got {T}")
    nb = T // 2
    ncol = max(1, -(-nb // SPECTRUM_BINS))
    tpad = -(-T // SPECTRUM_BK) * SPECTRUM_BK
    tab = np.zeros((tpad, ncol, 2, SPECTRUM_BINS), dtype=np.float64)
    k = np.arange(1, ncol * SPECTRUM_BINS + 1, dtype=np.int64)
    ang = 2.0 * np.pi * ((np.arange(T, dtype=np.int64)[:, None] * k[None, :]) % T).astype(np.float64) / T
    live = (k <= nb)[None, :]
    tab[:T, :, 0] = np.where(live, np.cos(ang), 0.0).reshape(T, ncol, SPECTRUM_BINS)
    tab[:T, :, 1] = np.where(live, np.sin(ang), 0.0).reshape(T, ncol, SPECTRUM_BINS)
    return torch.from_numpy(tab.reshape(tpad, ncol * 2 * SPECTRUM_BINS).astype(np.float32))


def _twiddles_on(T: int, device) -> torch.Tensor:
    key = (T, torch.device(device))
    if key not in _twiddle_cache:
        _twiddle_cache[key] = spectrum_twiddles(T).to(device)
    return _twiddle_cache[key]


def mirror_spectrum(half, T: int) -> np.ndarray:
    """bins 0 .. T // 2 ([..., T // 2 + 1]) -> the full length-T spectrum of a real series: bin T - k repeats bin k, the Nyquist bin of
    an even T appears once"""
    half = np.asarray(half, dtype=np.float64)
    if half.shape[-1] != T // 2 + 1:
        raise ValueError(f"a real series of {T} samples has {T // 2 + 1} bins, got {half.shape[-1]}")
    return np.concatenate([half, half[..., 1:(T + 1) // 2][..., ::-1]], axis=-1)


def spectrum_sums(x: torch.Tensor, mode: str = "gray", rescale: bool = True, luma=GRAY_LUMA):
    """The kernel's raw output, left on the device: (mag_sum, pow_sum) float64 [B, T // 2 + 1] - per-bin sums of |X_k| and |X_k|^2 over
    all series - and the series count (H W in gray mode, C H W in raw mode).  Nothing is synchronised."""
    _check_video(x, "x")
    if mode not in _SPECTRUM_MODES:
        raise _lib.HVKernelError(f"temporal spectrum: mode is 'gray' or 'raw', got {mode!r}")
    if x.dim() == 4:
        x = x[None]
    B, C, T, H, W = x.shape
    if mode == "gray" and C != 3:
        raise _lib.HVKernelError(f"temporal spectrum: gray mode reads RGB videos, got C = {C}")
    if not 1 <= T <= SPECTRUM_MAX_T:
        raise _lib.HVKernelError(f"temporal spectrum: 1 <= T <= {SPECTRUM_MAX_T}, got {T}")
    m = _SPECTRUM_MODES[mode]
    ws_bytes = _lib.host("temporal_spectrum_workspace_bytes", m, C, T, H, W)
    if ws_bytes <= 0:
        raise _lib.HVKernelError(f"temporal spectrum: unsupported shape {tuple(x.shape)} in {mode} mode")
    dev = x.device
    tw = _twiddles_on(T, dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    mag = torch.empty(B, T // 2 + 1, dtype=torch.float64, device=dev)
    pw = torch.empty(B, T // 2 + 1, dtype=torch.float64, device=dev)
    wr, wg, wb, rnd, shift = (int(v) for v in luma)
    for b in range(B):                        # one stream: video b + 1 reuses the workspace after video b's fold
        v = x[b]
        _lib.call("temporal_spectrum", v, v.stride(0), v.stride(1), v.stride(2), _DTYPES[x.dtype], m, C, T, H, W, 1 if rescale else 0,
                  wr, wg, wb, rnd, shift, tw, tw.numel(), mag[b], pw[b], ws, ws.numel())
    return mag, pw, (H * W if mode == "gray" else C * H * W)


def _spectra_to_host(jobs, fps_of):
    """jobs: [(mag_sum, pow_sum, series, T, batched)] on one device -> one synchronisation, then the host rules: divide by the series
    count, mirror"""
    host = []
    for mag, pw, _, _, _ in jobs:
        pair = []
        for t in (mag, pw):
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            pair.append(h)
        host.append(pair)
    torch.cuda.current_stream(jobs[0][0].device).synchronize()
    out = []
    for i, ((_, _, n, T, batched), (hm, hp)) in enumerate(zip(jobs, host)):
        mag, pw = mirror_spectrum(hm.numpy() / float(n), T), mirror_spectrum(hp.numpy() / float(n), T)
        if not batched:
            mag, pw = mag[0], pw[0]
        d = {"magnitude": mag, "power": pw}
        dt = fps_of(i)
        if dt is not None:
            d["freq"] = np.fft.fftfreq(T, dt)
        out.append(d)
    return out


def temporal_spectrum(x: torch.Tensor, mode: str = "gray", rescale: bool = True, fps: float = None, luma=GRAY_LUMA) -> dict:
    """Mean temporal spectrum of `x` ([C,T,H,W] or [B,C,T,H,W]; GPU tensors only, fp16 or fp32, W contiguous, strided views allowed, T <=
    1024), theory_analysis.ipynb cells 2 / 4.  mode "gray" (C = 3): one series per pixel of the 8-bit gray frame - the bytes
    `frames_uint8` writes (rescale: values in [-1, 1], else [0, 1]) under the integer luma `luma` = (wr, wg, wb, round, shift), default
    GRAY_LUMA: OpenCV's 8-bit BGR2GRAY rule as restated here, NOT pinned against cv2 (which this environment lacks).  mode "raw": one
    series per (c, h, w), values as they are (the latent mean).  Returns float64 numpy arrays `magnitude` [T] ([B,T] for a batch) - the
    reference's np.abs(np.fft.fft(signal, axis=0)).mean(axis=1), bin 0 included, mirrored to full length -, `power` [T], the mean
    |X_k|^2, and with `fps` `freq` = np.fft.fftfreq(T, 1 / fps).  One host synchronisation."""
    batched = isinstance(x, torch.Tensor) and x.dim() == 5
    mag, pw, n = spectrum_sums(x, mode, rescale, luma)
    T = x.shape[-3]
    return _spectra_to_host([(mag, pw, n, T, batched)], lambda i: None if fps is None else 1.0 / fps)[0]


def high_band_share(power, cutoff_bin: int) -> float:
    """Share of the non-DC power of a full-length spectrum `power` [T] that sits at bins cutoff_bin <= k <= T - cutoff_bin (both mirror
    images of the band; the Nyquist bin of an even T is counted once).  0.0 when there is no non-DC power or the band is empty."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim != 1:
        raise ValueError(f"high_band_share takes one spectrum [T], got shape {p.shape}")
    T = p.shape[0]
    if cutoff_bin < 1:
        raise ValueError(f"cutoff_bin must be >= 1 (bin 0 is the DC term), got {cutoff_bin}")
    total = float(p[1:].sum())
    if total <= 0.0 or cutoff_bin > T - cutoff_bin:
        return 0.0
    return float(p[cutoff_bin:T - cutoff_bin + 1].sum()) / total


def latent_nyquist_bin(T: int, T_in: int, T_lat: int) -> int:
    """The first bin k of a length-T spectrum with k / T >= 1 / (2 T_in / T_lat): the Nyquist frequency of a latent that keeps T_lat
    samples of T_in frames, in cycles per frame"""
    return max(1, -(-T * T_lat // (2 * T_in)))


def spectrum_report(clip: torch.Tensor, latent: torch.Tensor, recon: torch.Tensor, fps: float = None, t_ratio: int = 4,
                    rescale: bool = True) -> dict:
    """The three spectra of one reconstruction and what each loses: {"input", "reconstruction", "latent"}, each the dict of
    `temporal_spectrum` (gray mode for `clip` and `recon`, raw mode for `latent`) plus `high_band_share` and `cutoff_bin`.  The videos'
    cutoff is the Nyquist bin of the latent rate (`latent_nyquist_bin` with T_in, T_lat of `clip` and `latent`): what a temporal
    pool, stride or interpolation down to T_lat samples cannot carry.  The latent's own cutoff is the upper half of its band (the first
    bin with k / T_lat >= 1 / 4).  With `fps` the videos get freq = fftfreq(T, 1 / fps) and the latent fftfreq(T_lat, t_ratio / fps), as
    cell 4.  Batches give one share per video.  All launches are enqueued first: one host synchronisation."""
    items = (("input", clip, "gray"), ("latent", latent, "raw"), ("reconstruction", recon, "gray"))
    jobs = []
    for _, x, mode in items:
        mag, pw, n = spectrum_sums(x, mode, rescale)
        jobs.append((mag, pw, n, x.shape[-3], x.dim() == 5))
    dts = [None if fps is None else (t_ratio / fps if mode == "raw" else 1.0 / fps) for _, _, mode in items]
    out = {name: d for (name, _, _), d in zip(items, _spectra_to_host(jobs, lambda i: dts[i]))}
    return add_high_band_shares(out)


def add_high_band_shares(spectra: dict) -> dict:
    """`cutoff_bin` and `high_band_share` for the {"input", "latent", "reconstruction"} spectra of `spectrum_report` (pure numpy): the
    frame counts are the lengths of the spectra themselves"""
    T_in, T_lat = spectra["input"]["power"].shape[-1], spectra["latent"]["power"].shape[-1]
    for name, d in spectra.items():
        T = d["power"].shape[-1]
        cut = max(1, -(-T // 4)) if name == "latent" else latent_nyquist_bin(T, T_in, T_lat)
        d["cutoff_bin"] = cut
        d["high_band_share"] = (float(high_band_share(d["power"], cut)) if d["power"].ndim == 1
                                else np.array([high_band_share(p, cut) for p in d["power"]]))
    return spectra


def spectrum_json(report: dict) -> dict:
    """a `spectrum_report` of ONE video as plain lists and floats (the <name>_spectrum.json of infer.py --spectrum)"""
    return {name: {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()} for name, d in report.items()}


# ---- content statistics and buckets (csrc/hv_content.hip) -------------------------------------------------------------------------------
# The last stage of the fork's study, run_experiments_buckets.sh, runs every configuration once per content bucket; the buckets are lists
# named after a measure and its edges (metric_buckets/InterEntropy_buckets/Very_Low_InterEntropy_lt2.txt, Low_InterEntropy_2-4.txt,
# Medium_InterEntropy_4-6.txt).  The fork does not contain the program that computed the measure, so the definition below is this
# project's own and every record that carries a value says so.
CONTENT_DEFINITION = ("entropy of the 8-bit gray frame difference histogram, bits; this project's definition, the fork publishes only "
                      "the bucket names")
CONTENT_INTER_BINS, CONTENT_CHUNK = _abi.CONTENT_MACROS["HV_CONTENT_INTER_BINS"], _abi.CONTENT_MACROS["HV_CONTENT_CHUNK"]
CONTENT_EDGES = (2.0, 4.0, 6.0)
# (label = the fork's file stem, lower edge, upper edge): half-open [lo, hi); the fork's three, then everything above its last edge
CONTENT_BUCKETS = (("Very_Low_InterEntropy_lt2", None, 2.0), ("Low_InterEntropy_2-4", 2.0, 4.0), ("Medium_InterEntropy_4-6", 4.0, 6.0),
                   ("High_InterEntropy_gt6", 6.0, None))


_BUCKET_WORDS = {"inter": "InterEntropy", "intra": "IntraEntropy", "motion": "Motion"}


def _edge_text(v) -> str:
    return f"{float(v):g}"


def content_bucket_labels(edges=CONTENT_EDGES, metric: str = "inter"):
    """the bucket labels for `edges` (ascending), lowest first: the fork's names for its own edges (2, 4, 6), the same pattern for others:
    Very_Low / Low / Medium / High for four buckets, B<i> otherwise; `metric` "inter" | "intra" | "motion" names the measure (`Motion`:
    `motion_mean` of `motion_stats`, px/frame; its edges have no default - nobody has measured natural clips under that definition)"""
    edges = [float(e) for e in edges]
    if not edges or any(b <= a for a, b in zip(edges, edges[1:])):
        raise ValueError(f"bucket edges must be ascending and not empty, got {edges}")
    if metric not in _BUCKET_WORDS:
        raise ValueError(f"metric is 'inter', 'intra' or 'motion', got {metric!r}")
    word = _BUCKET_WORDS[metric]
    n = len(edges) + 1
    ranks = ("Very_Low", "Low", "Medium", "High") if n == 4 else tuple(f"B{i}" for i in range(n))
    out = []
    for i in range(n):
        span = f"lt{_edge_text(edges[0])}" if i == 0 else f"gt{_edge_text(edges[-1])}" if i == n - 1 else \
            f"{_edge_text(edges[i - 1])}-{_edge_text(edges[i])}"
        out.append(f"{ranks[i]}_{word}_{span}")
    return out


def content_bucket(value, edges=CONTENT_EDGES, metric: str = "inter"):
    """The label of the bucket `value` falls in, half-open intervals [lo, hi): the fork's `lt2` is strictly below 2, exactly 2.0 is
    `Low_InterEntropy_2-4`.  None (a single-frame clip has no inter-frame entropy) and NaN belong to no bucket: None."""
    labels = content_bucket_labels(edges, metric)
    if value is None or value != value:
        return None
    i = 0
    for e in edges:
        if float(value) >= float(e):
            i += 1
    return labels[i]


def _content_check(x, luma):
    _check_video(x, "x")
    if x.shape[-4] != 3:
        raise _lib.HVKernelError(f"content histograms read RGB videos, got C = {x.shape[-4]}")
    if len(tuple(luma)) != 5:
        raise _lib.HVKernelError(f"luma is (wr, wg, wb, round, shift), got {luma!r}")


def content_histograms(x: torch.Tensor, rescale: bool = True, luma=GRAY_LUMA):
    """Histograms of the 8-bit gray frames of `x` ([3,T,H,W] or [B,3,T,H,W]; GPU tensors only, fp16 or fp32, W contiguous, strided views
    allowed; gray as in `temporal_spectrum`'s gray mode) and of the differences of consecutive gray frames, left on the device:
    `intra` int32 [T, 256] - pixels of frame t with gray value g - and `inter` int32 [T - 1, 511] - pixels with gray[t + 1] - gray[t] ==
    d in column d + 255 ([B, ...] for a batch).  Counts are exact (at most H W <= 2^31 - 1).  Nothing is synchronised."""
    _content_check(x, luma)
    batched = x.dim() == 5
    if not batched:
        x = x[None]
    B, _, T, H, W = x.shape
    ws_bytes = _lib.host("content_histograms_workspace_bytes", T, H, W)
    if ws_bytes <= 0:
        raise _lib.HVKernelError(f"content histograms: unsupported shape {tuple(x.shape)}")
    dev = x.device
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    intra = torch.empty(B, T, 256, dtype=torch.int32, device=dev)
    inter = torch.empty(B, T - 1, CONTENT_INTER_BINS, dtype=torch.int32, device=dev)
    wr, wg, wb, rnd, shift = (int(v) for v in luma)
    for b in range(B):                        # one stream: video b + 1 reuses the workspace after video b's fold
        v = x[b]
        _lib.call("content_histograms", v, v.stride(0), v.stride(1), v.stride(2), _DTYPES[x.dtype], T, H, W, 1 if rescale else 0,
                  wr, wg, wb, rnd, shift, intra[b], inter[b] if T > 1 else None, ws, ws.numel())
    return (intra, inter) if batched else (intra[0], inter[0])


def histogram_entropy(counts: torch.Tensor, origin: int = 0) -> torch.Tensor:
    """float64 [rows, 3] on the device: (entropy in bits, sum c v, sum c v^2) of every row of `counts` (int32 [rows, bins <= 1024], GPU,
    contiguous), bin b standing for the value b - origin.  Nothing is synchronised."""
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
        raise _lib.HVKernelError("histogram_entropy: expected a GPU tensor (this package has no CPU path)")
    if counts.dtype != torch.int32 or counts.dim() != 2 or not counts.is_contiguous():
        raise _lib.HVKernelError(f"histogram_entropy: counts are contiguous int32 [rows, bins], got {counts.dtype} {tuple(counts.shape)}")
    rows, bins = counts.shape
    out = torch.empty(rows, 3, dtype=torch.float64, device=counts.device)
    if rows:
        _lib.call("histogram_entropy", counts, rows, bins, int(origin), out)
    return out


def _content_enqueue(x: torch.Tensor, rescale: bool = True, luma=GRAY_LUMA):
    """histograms and their entropies of ONE clip ([3,T,H,W] or [1,3,T,H,W]), everything enqueued, nothing synchronised: a job for
    `_content_to_host`"""
    _content_check(x, luma)
    if x.dim() == 5:
        if x.shape[0] != 1:
            raise _lib.HVKernelError(f"content entropy takes one clip at a time, got a batch of {x.shape[0]}")
        x = x[0]
    intra, inter = content_histograms(x, rescale, luma)
    return (histogram_entropy(intra, 0), histogram_entropy(inter, 255), inter, x.shape[-3], x.shape[-2] * x.shape[-1])


def content_from_host(intra_stats, inter_stats, inter_counts, frames: int, pixels: int) -> dict:
    """The host rules on the finaliser's rows (numpy float64; pure, also used on CPU by the tests): intra_stats [T, 3], inter_stats
    [T - 1, 3] = (entropy, sum c v, sum c v^2) per row, inter_counts [T - 1, 511]."""
    intra_stats = np.asarray(intra_stats, dtype=np.float64).reshape(-1, 3)
    inter_stats = np.asarray(inter_stats, dtype=np.float64).reshape(-1, 3)
    inter_counts = np.asarray(inter_counts, dtype=np.int64).reshape(-1, CONTENT_INTER_BINS)
    n = float(pixels)
    d = {"inter_entropy": None, "intra_entropy": float(intra_stats[:, 0].mean()), "intra_entropy_frames": intra_stats[:, 0].tolist(),
         "inter_entropy_pairs": inter_stats[:, 0].tolist(), "mean_abs_diff": None, "ti": None, "frames": int(frames),
         "definition": CONTENT_DEFINITION}
    if inter_stats.shape[0]:
        d["inter_entropy"] = float(inter_stats[:, 0].mean())
        absv = np.abs(np.arange(CONTENT_INTER_BINS, dtype=np.int64) - 255)
        d["mean_abs_diff"] = float(((inter_counts * absv[None, :]).sum(axis=1) / n).mean())
        # ITU-T P.910 temporal information: max over time of the spatial standard deviation of the difference; the moments are exact
        # integers (below 2^53 as doubles), so the variance (N S2 - S1^2) / N^2 is formed in python integers and rounded once
        var = [(int(pixels) * int(s2) - int(s1) * int(s1)) / float(int(pixels) ** 2) for _, s1, s2 in inter_stats]
        d["ti"] = math.sqrt(max(var))
    return d


def _content_to_host(jobs):
    """jobs of `_content_enqueue` on one device -> one synchronisation, then `content_from_host` per job"""
    host = []
    for job in jobs:
        trio = []
        for t in job[:3]:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            trio.append(h)
        host.append(trio)
    torch.cuda.current_stream(jobs[0][0].device).synchronize()
    return [content_from_host(hi.numpy(), hp.numpy(), hc.numpy(), job[3], job[4]) for job, (hi, hp, hc) in zip(jobs, host)]


def content_entropy(x: torch.Tensor, rescale: bool = True, luma=GRAY_LUMA) -> dict:
    """Content statistics of one clip ([3,T,H,W] or [1,3,T,H,W], as `content_histograms`): `inter_entropy` - the mean over the T - 1 frame
    pairs of the Shannon entropy, in bits, of the histogram of gray[t + 1] - gray[t] (None for T = 1: such a clip is not bucketed) -,
    `intra_entropy` - the mean over frames of the entropy of the gray histogram -, the per-pair and per-frame lists
    (`inter_entropy_pairs`, `intra_entropy_frames`), `mean_abs_diff` (mean |difference| in gray levels, mean over pairs), `ti` (ITU-T
    P.910 temporal information: the maximum over pairs of the standard deviation of the difference, from exact integer moments),
    `frames`, and `definition` (CONTENT_DEFINITION: the measure is this project's own).  One host synchronisation."""
    return _content_to_host([_content_enqueue(x, rescale, luma)])[0]


def content_entropy_many(clips, rescale: bool = True, luma=GRAY_LUMA) -> list:
    """`content_entropy` of every clip of an iterable (a generator may load and drop one clip at a time: only the histograms of a clip
    outlive its launches), everything enqueued first: one host synchronisation for all of them"""
    jobs = [_content_enqueue(x, rescale, luma) for x in clips]
    return _content_to_host(jobs) if jobs else []


_CONTENT_MEANS = ("inter_entropy", "intra_entropy", "mean_abs_diff", "ti")


def content_summary(inputs: list, recons: list) -> dict:
    """The `content` entry of a driver's record: the fields of `content_entropy` averaged over the clips that have them, for the inputs
    and for their reconstructions, and `inter_entropy_drop` = input - reconstruction: the frame-to-frame detail a pool or stride removed"""
    def mean(ds, k):
        v = [d[k] for d in ds if d[k] is not None]
        return sum(v) / len(v) if v else None
    out = {"input": {k: mean(inputs, k) for k in _CONTENT_MEANS}, "reconstruction": {k: mean(recons, k) for k in _CONTENT_MEANS},
           "clips": len(inputs), "definition": CONTENT_DEFINITION}
    a, b = out["input"]["inter_entropy"], out["reconstruction"]["inter_entropy"]
    out["inter_entropy_drop"] = None if a is None or b is None else a - b
    return out


# ---- block-matching motion fields (csrc/hv_motion.hip) ---------------------------------------------------------------------------------
# The fork's per-video table has an `fvdm` column (FVMD: keypoint tracks of a third-party tracker) and its dataset tool a `large_motion`
# folder; neither program is in the fork.  What follows is NOT FVMD and fills no `fvdm` column: it is dense full-search block matching on
# the 8-bit gray frames, a measure of this project's own, and every record that carries a value says so.
MOTION_DEFINITION = ("full-search block matching on 8-bit gray frames (SAD + lam (|dy| + |dx|), ties to the shorter vector), px/frame; "
                     "this project's own measure, not FVMD")
MOTION_MAX_RADIUS, MOTION_MAX_LAM = _abi.MOTION_MACROS["HV_MOTION_MAX_RADIUS"], _abi.MOTION_MACROS["HV_MOTION_MAX_LAM"]
MOTION_BLOCKS = (8, 16)


def motion_default_lam(block: int) -> int:
    """block * block // 16: a displacement of one pixel must gain 1/16 gray code per pixel of the block to be taken.  This project's
    choice (there is no reference to take it from)."""
    return int(block) * int(block) // 16


def _motion_params(block, radius, lam):
    block, radius = int(block), int(radius)
    if block not in MOTION_BLOCKS:
        raise ValueError(f"motion block is 8 or 16, got {block}")
    if not 1 <= radius <= MOTION_MAX_RADIUS:
        raise ValueError(f"motion radius is in [1, {MOTION_MAX_RADIUS}], got {radius}")
    lam = motion_default_lam(block) if lam is None else int(lam)
    if not 0 <= lam <= MOTION_MAX_LAM:
        raise ValueError(f"motion lam is in [0, {MOTION_MAX_LAM}], got {lam}")
    return block, radius, lam


def block_motion(x: torch.Tensor, block: int = 16, radius: int = 16, lam: int = None, rescale: bool = True, luma=GRAY_LUMA):
    """The motion field of one clip `x` ([3,T,H,W] or [1,3,T,H,W]; GPU tensors only, fp16 or fp32, W contiguous, strided views allowed;
    gray as in `content_histograms`), left on the device: for every pair of consecutive frames and every `block` x `block` block of the
    later frame (edge blocks partial) the displacement (dy, dx) in [-radius, radius]^2 into the earlier frame (replicated edges) that
    minimises SAD + lam (|dy| + |dx|), ties to the smaller dy^2 + dx^2, then dy, then dx.  -> `mv` int16 [T-1, Hb, Wb, 2], `sad` int32
    [T-1, Hb, Wb] (the winner's SAD without the penalty), `sad0` int32 (the SAD at (0, 0)).  `lam` None = `motion_default_lam(block)`.
    Exact integers; this project's own measure, not FVMD.  Nothing is synchronised."""
    _content_check(x, luma)
    block, radius, lam = _motion_params(block, radius, lam)
    if x.dim() == 5:
        if x.shape[0] != 1:
            raise _lib.HVKernelError(f"block_motion takes one clip at a time, got a batch of {x.shape[0]}")
        x = x[0]
    _, T, H, W = x.shape
    Hb, Wb = -(-H // block), -(-W // block)
    dev = x.device
    mv = torch.empty(T - 1, Hb, Wb, 2, dtype=torch.int16, device=dev)
    sad = torch.empty(T - 1, Hb, Wb, dtype=torch.int32, device=dev)
    sad0 = torch.empty(T - 1, Hb, Wb, dtype=torch.int32, device=dev)
    wr, wg, wb, rnd, shift = (int(v) for v in luma)
    pair = T > 1
    _lib.call("block_motion", x, x.stride(0), x.stride(1), x.stride(2), _DTYPES[x.dtype], T, H, W, 1 if rescale else 0, wr, wg, wb, rnd,
              shift, block, radius, lam, mv if pair else None, sad if pair else None, sad0 if pair else None)
    return mv, sad, sad0


def motion_epe(mv_a, mv_b) -> float:
    """mean Euclidean distance between two vector fields of one shape [P, Hb, Wb, 2] (numpy float64); None without pairs"""
    a, b = np.asarray(mv_a, dtype=np.float64), np.asarray(mv_b, dtype=np.float64)
    if a.shape != b.shape:
        raise ValueError(f"motion fields of different shapes: {a.shape}, {b.shape}")
    if a.size == 0:
        return None
    return float(np.sqrt(((a - b) ** 2).sum(axis=-1)).mean())


def motion_from_host(mv, sad, sad0, radius: int, block: int = None, lam: int = None) -> dict:
    """The host rules on a motion field (numpy float64; pure, also used on CPU by the tests): mv [P, Hb, Wb, 2] = (dy, dx), sad and sad0
    [P, Hb, Wb].  `motion_mean` - the mean over pairs of the mean over blocks of sqrt(dy^2 + dx^2), px/frame -, `motion_pairs` (per
    pair), `motion_max`, `static_share` (blocks at (0, 0)), `border_share` (blocks with |dy| or |dx| at the radius: the search was too
    small for them), `mc_gain` = 1 - sum sad / sum sad0 (0 when sum sad0 is 0), `frames`, `block`, `radius`, `lam`, `definition`.  Without
    pairs (a single frame) the values are None."""
    mv = np.asarray(mv, dtype=np.int64)
    if mv.ndim != 4 or mv.shape[-1] != 2:
        raise ValueError(f"a motion field is [pairs, Hb, Wb, 2], got {mv.shape}")
    P = mv.shape[0]
    d = {"motion_mean": None, "motion_pairs": [], "motion_max": None, "static_share": None, "border_share": None, "mc_gain": None,
         "frames": P + 1, "block": None if block is None else int(block), "radius": int(radius), "lam": None if lam is None else int(lam),
         "definition": MOTION_DEFINITION}
    if P == 0:
        return d
    dy, dx = mv[..., 0], mv[..., 1]
    mag = np.sqrt((dy * dy + dx * dx).astype(np.float64))
    pairs = mag.reshape(P, -1).mean(axis=1)
    s, s0 = int(np.asarray(sad, dtype=np.int64).sum()), int(np.asarray(sad0, dtype=np.int64).sum())
    d.update(motion_mean=float(pairs.mean()), motion_pairs=pairs.tolist(), motion_max=float(mag.max()),
             static_share=float(((dy == 0) & (dx == 0)).mean()),
             border_share=float(((np.abs(dy) == int(radius)) | (np.abs(dx) == int(radius))).mean()),
             mc_gain=(1.0 - s / s0) if s0 else 0.0)
    return d


def _motion_enqueue(x: torch.Tensor, block: int = 16, radius: int = 16, lam: int = None, rescale: bool = True, luma=GRAY_LUMA):
    """the field of ONE clip, enqueued, nothing synchronised: a job for `_motion_to_host`"""
    block, radius, lam = _motion_params(block, radius, lam)
    return (*block_motion(x, block, radius, lam, rescale, luma), block, radius, lam)


def _motion_to_host(jobs):
    """jobs of `_motion_enqueue` on one device -> one synchronisation -> per job the host field {"mv", "sad", "sad0", "block", "radius",
    "lam"} (numpy)"""
    host = []
    for job in jobs:
        trio = []
        for t in job[:3]:
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            trio.append(h)
        host.append(trio)
    torch.cuda.current_stream(jobs[0][0].device).synchronize()
    return [{"mv": m.numpy(), "sad": s.numpy(), "sad0": s0.numpy(), "block": job[3], "radius": job[4], "lam": job[5]}
            for job, (m, s, s0) in zip(jobs, host)]


def motion_field_stats(field: dict, pairs: int = None) -> dict:
    """`motion_from_host` of a host field of `_motion_to_host`, of its first `pairs` pairs when given (a pair depends on its two frames
    only, so the rows of a longer clip are the rows of its prefix)"""
    p = slice(None) if pairs is None else slice(0, pairs)
    return motion_from_host(field["mv"][p], field["sad"][p], field["sad0"][p], field["radius"], field["block"], field["lam"])


def motion_stats(x: torch.Tensor, block: int = 16, radius: int = 16, lam: int = None, rescale: bool = True, luma=GRAY_LUMA) -> dict:
    """How much one clip moves ([3,T,H,W] or [1,3,T,H,W], as `block_motion`): the dict of `motion_from_host`.  One host
    synchronisation.  This project's own measure, not FVMD."""
    return motion_field_stats(_motion_to_host([_motion_enqueue(x, block, radius, lam, rescale, luma)])[0])


def motion_stats_many(clips, block: int = 16, radius: int = 16, lam: int = None, rescale: bool = True, luma=GRAY_LUMA) -> list:
    """`motion_stats` of every clip of an iterable (a generator may load and drop one clip at a time: only the fields outlive the
    launches), everything enqueued first: one host synchronisation for all of them"""
    jobs = [_motion_enqueue(x, block, radius, lam, rescale, luma) for x in clips]
    return [motion_field_stats(f) for f in _motion_to_host(jobs)] if jobs else []


def motion_compare_fields(ref_field: dict, rec_field: dict) -> dict:
    """two host fields of one geometry -> {"ref", "rec"} (`motion_from_host` of each over the pairs both have), `motion_epe` (the mean
    Euclidean distance between the two vector fields, px) and `motion_mean_change` = rec - ref"""
    if any(ref_field[k] != rec_field[k] for k in ("block", "radius", "lam")) or ref_field["mv"].shape[1:] != rec_field["mv"].shape[1:]:
        raise ValueError("motion fields of different geometry")
    P = min(ref_field["mv"].shape[0], rec_field["mv"].shape[0])
    a, b = motion_field_stats(ref_field, P), motion_field_stats(rec_field, P)
    change = None if a["motion_mean"] is None else b["motion_mean"] - a["motion_mean"]
    return {"ref": a, "rec": b, "motion_epe": motion_epe(ref_field["mv"][:P], rec_field["mv"][:P]), "motion_mean_change": change,
            "definition": MOTION_DEFINITION}


def _motion_pair_check(ref, rec):
    """the rules of the pair scorers (`video_stats`): one dtype, one device, shapes equal but for the frame count -> (ref, rec) as
    [3,T,H,W] cut to the frames both have"""
    _check_video(ref, "ref"), _check_video(rec, "rec")
    if ref.dim() == 5 and ref.shape[0] == 1:
        ref = ref[0]
    if rec.dim() == 5 and rec.shape[0] == 1:
        rec = rec[0]
    if ref.dim() != 4 or rec.dim() != 4:
        raise _lib.HVKernelError(f"motion_compare takes one clip and one reconstruction, got {tuple(ref.shape)} and {tuple(rec.shape)}")
    if ref.dtype != rec.dtype:
        raise _lib.HVKernelError(f"ref and rec must have one dtype, got {ref.dtype} and {rec.dtype}")
    if ref.device != rec.device:
        raise _lib.HVKernelError(f"ref and rec are on different devices: {ref.device}, {rec.device}")
    if (ref.shape[0], ref.shape[2], ref.shape[3]) != (rec.shape[0], rec.shape[2], rec.shape[3]):
        raise _lib.HVKernelError(f"ref {tuple(ref.shape)} and rec {tuple(rec.shape)} differ in more than the frame count")
    T = min(ref.shape[1], rec.shape[1])
    return ref[:, :T], rec[:, :T]


def motion_compare(ref: torch.Tensor, rec: torch.Tensor, block: int = 16, radius: int = 16, lam: int = None, rescale: bool = True,
                   luma=GRAY_LUMA) -> dict:
    """Does the reconstruction move as its input does: both clips' `motion_stats` over the first min(T_ref, T_rec) frames (the pair
    scorers' rule) plus `motion_epe` and `motion_mean_change` (`motion_compare_fields`).  One host synchronisation."""
    ref, rec = _motion_pair_check(ref, rec)
    a, b = _motion_to_host([_motion_enqueue(ref, block, radius, lam, rescale, luma), _motion_enqueue(rec, block, radius, lam, rescale, luma)])
    return motion_compare_fields(a, b)


_MOTION_MEANS = ("motion_mean", "motion_max", "static_share", "border_share", "mc_gain")


def motion_summary(inputs: list, compares: list) -> dict:
    """The `motion` entry of a driver's record: the fields of `motion_stats` averaged over the clips that have them, for the inputs
    (`inputs`: their `motion_stats`) and for the reconstructions (`compares`: the `motion_compare` results), and the means of
    `motion_epe` and `motion_mean_change`"""
    def mean(ds, k):
        v = [d[k] for d in ds if d[k] is not None]
        return sum(v) / len(v) if v else None
    recs = [c["rec"] for c in compares]
    first = (inputs or recs or [{}])[0]
    return {"input": {k: mean(inputs, k) for k in _MOTION_MEANS}, "reconstruction": {k: mean(recs, k) for k in _MOTION_MEANS},
            "motion_epe": mean(compares, "motion_epe"), "motion_mean_change": mean(compares, "motion_mean_change"), "clips": len(inputs),
            "block": first.get("block"), "radius": first.get("radius"), "lam": first.get("lam"), "definition": MOTION_DEFINITION}


def add_motion_arguments(parser):
    """--motion [--motion-block 8|16] [--motion-radius R] [--motion-lam L]: the block-matching motion score of the drivers"""
    parser.add_argument("--motion", action="store_true", help="block-matching motion fields of input and reconstruction (mean px/frame, "
                                                              "end-point error between the two fields); this project's own measure, not FVMD")
    parser.add_argument("--motion-block", type=int, default=None, choices=MOTION_BLOCKS, help="with --motion: block size (default 16)")
    parser.add_argument("--motion-radius", type=int, default=None, help=f"with --motion: search radius, 1..{MOTION_MAX_RADIUS} (default 16)")
    parser.add_argument("--motion-lam", type=int, default=None, help=f"with --motion: penalty per pixel of |dy| + |dx|, 0..{MOTION_MAX_LAM} "
                                                                     "(default block * block // 16)")


def motion_from_args(args, parser):
    """-> None without --motion, else {"block", "radius", "lam"}; the sub-flags without --motion and values out of range are errors"""
    sub = [f for f, v in (("--motion-block", args.motion_block), ("--motion-radius", args.motion_radius), ("--motion-lam", args.motion_lam))
           if v is not None]
    if not args.motion:
        if sub:
            parser.error(f"{', '.join(sub)} only valid with --motion")
        return None
    try:
        block, radius, lam = _motion_params(16 if args.motion_block is None else args.motion_block,
                                            16 if args.motion_radius is None else args.motion_radius, args.motion_lam)
    except ValueError as e:
        parser.error(str(e))
    return {"block": block, "radius": radius, "lam": lam}


def add_lpips_arguments(parser, synthetic: bool = False):
    """--lpips-alexnet PATH [--lpips-linear PATH] (and --lpips-synthetic for the tools that have a synthetic-weight mode)"""
    parser.add_argument("--lpips-alexnet", type=str, default=None, help="score LPIPS too: a torchvision AlexNet state dict (needs "
                        "--lpips-linear), or one full LPIPS state dict (.pt / .pth / .safetensors; weights are not shipped)")
    parser.add_argument("--lpips-linear", type=str, default=None, help="the LPIPS linear layers (lin{0..4}.model.1.weight), e.g. lpips' weights/v0.1/alex.pth")
    if synthetic:
        parser.add_argument("--lpips-synthetic", action="store_true", help="score LPIPS under deterministic synthetic weights: exercises the "
                            "kernels; the value is NOT comparable with published LPIPS")


def lpips_from_args(args, parser=None):
    """the LpipsAlex the flags of add_lpips_arguments ask for, or None"""
    def fail(msg):
        if parser is not None:
            parser.error(msg)
        raise ValueError(msg)
    synthetic = bool(getattr(args, "lpips_synthetic", False))
    if args.lpips_linear and not args.lpips_alexnet:
        fail("--lpips-linear needs --lpips-alexnet")
    if synthetic and args.lpips_alexnet:
        fail("--lpips-synthetic and --lpips-alexnet exclude each other")
    if synthetic:
        print("LPIPS: synthetic weights - the LPIPS value is not comparable with published LPIPS")
        return LpipsAlex.synthetic(0)
    if args.lpips_alexnet:
        return LpipsAlex.from_files(args.lpips_alexnet, args.lpips_linear)
    return None


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


METRICS_CSV_HEADER = ["video_path", "ssim", "psnr", "lpips", "fvd", "fvdm"]


def add_gssim_arguments(parser, csv: bool = True):
    parser.add_argument("--gssim", action="store_true", help="score the Gaussian-window SSIMs of the fork's rebuttal tables too: SSIM3D "
                        "(run.py: pytorch_msssim on [B,C,T,H,W], the window spans T) and SSIM2D (calculate_ssim.py: per frame)")
    if csv:
        parser.add_argument("--metrics-csv", type=str, default=None, help="write one row per clip under run.py's header (video_path, ssim, "
                            "psnr, lpips, fvd, fvdm); ssim is SSIM3D; fvd and fvdm stay empty (styleganv detector / keypoint tracker: "
                            "out of scope)")


class MetricsAccumulator:
    """Per-frame scores of many videos; the experiment's number is the mean over all FRAMES (compute_metrics.py:150-154), so a long
    video weighs more than a short one.  `lpips` (an LpipsAlex): add_video scores LPIPS too (compute_metrics.py:142-146,153-154)."""

    def __init__(self, lpips: "LpipsAlex" = None, fvd: "I3D" = None, gssim: bool = False, csv: bool = False):
        """`gssim`: add_video scores the two Gaussian-window SSIMs too and result() gains "SSIM3D", "SSIM2D".  `csv`: add_video(names=)
        also keeps one row per clip for save_csv (the Gaussian-window scores are computed for it, result() is unchanged by it)."""
        self.psnr, self.ssim, self.lpips = [], [], []
        self.gssim = gssim
        self.csv = csv
        self.csv_rows = []
        self.ssim3d, self.ssim2d = [], []          # with gssim: one value of each Gaussian-window score per clip
        self.lpips_model = lpips
        self.fvd_model = fvd
        self.fvd_ref, self.fvd_rec = [], []        # one I3D logits vector [400] per input clip and per reconstruction
        self.motion = []                           # add_motion: one motion_compare result per clip pair

    def add_motion(self, compare: dict):
        """a `motion_compare` result of one clip pair: result() gains "MotionEPE" and "MotionMean" (means over the clips that have
        pairs of frames), present only once this was called"""
        self.motion.append(compare)

    def add(self, psnr, ssim, lpips=None):
        """per-frame arrays of one video (or a [B,T] batch), e.g. video_metrics(...)["psnr"], ["ssim"] (and ["lpips"])"""
        psnr, ssim = np.asarray(psnr, dtype=np.float64).ravel(), np.asarray(ssim, dtype=np.float64).ravel()
        if psnr.shape != ssim.shape:
            raise ValueError(f"psnr has {psnr.size} frames, ssim {ssim.size}")
        if lpips is not None:
            lpips = np.asarray(lpips, dtype=np.float64).ravel()
            if lpips.shape != psnr.shape:
                raise ValueError(f"psnr has {psnr.size} frames, lpips {lpips.size}")
            self.lpips.extend(lpips.tolist())
        self.psnr.extend(psnr.tolist())
        self.ssim.extend(ssim.tolist())

    def add_video(self, ref: torch.Tensor, rec: torch.Tensor, rescale: bool = True, ref_logits=None, names=None) -> dict:
        """`ref_logits` (with fvd=): the I3D logits of `ref` from an earlier call (m["fvd_ref_logits"]), which do not depend on how
        `rec` was made; they are computed here otherwise.  With fvd= a pair with fewer than 10 common frames is a ValueError, raised
        before anything of the pair is scored (the reference asserts the same): it is not skipped."""
        if self.fvd_model is not None and min(ref.shape[-3], rec.shape[-3]) < I3D_MIN_FRAMES:
            raise ValueError(f"fvd: a clip needs at least {I3D_MIN_FRAMES} frames, got {min(ref.shape[-3], rec.shape[-3])} common frames")
        m = video_metrics(ref, rec, rescale, lpips=self.lpips_model, gssim=self.gssim or self.csv)
        self.add(m["psnr"], m["ssim"], m.get("lpips"))
        if self.csv:
            if names is None:
                raise ValueError("an accumulator with csv=True needs add_video(names=[one path per clip])")
            rows = lambda v: np.asarray(v, dtype=np.float64).reshape(len(names), -1)      # noqa: E731
            lp = rows(m["lpips"]).mean(axis=1) if "lpips" in m else [""] * len(names)
            for name, s3, ps, l in zip(names, np.atleast_1d(m["ssim3d"]), rows(m["psnr"]).mean(axis=1), lp):
                self.csv_rows.append([name, float(s3), float(ps), l if l == "" else float(l), "", ""])
        if self.gssim:
            self.ssim3d.extend(np.atleast_1d(m["ssim3d"]).tolist())
            self.ssim2d.extend(np.atleast_1d(m["ssim2d"]).tolist())
        if self.fvd_model is not None:
            T = min(ref.shape[-3], rec.shape[-3])               # the frames the other scores saw
            lr = fvd_logits(ref[..., :T, :, :], self.fvd_model, rescale) if ref_logits is None else ref_logits
            m["fvd_ref_logits"] = lr
            m["fvd_rec_logits"] = fvd_logits(rec[..., :T, :, :], self.fvd_model, rescale)
            self.add_logits(lr, m["fvd_rec_logits"])
        return m

    def add_logits(self, ref_logits, rec_logits):
        """I3D logits [400] or [B,400] of input clips and of their reconstructions"""
        for dst, v in ((self.fvd_ref, ref_logits), (self.fvd_rec, rec_logits)):
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            dst.extend(np.asarray(v, dtype=np.float32).reshape(-1, I3D_CLASSES))

    @property
    def clips(self) -> int:
        return len(self.fvd_rec)

    @property
    def frames(self) -> int:
        return len(self.psnr)

    def result(self) -> dict:
        """{"PSNR": ..., "SSIM": ...}, only if LPIPS values were added "LPIPS", only with gssim "SSIM3D" and "SSIM2D", and only if the logits of at least two clip pairs were
        added "FVD" (FVD_LABEL: the Frechet distance between the inputs' and the reconstructions' I3D logits); empty when nothing was
        added (the reference writes no key then)."""
        out = {}
        if self.psnr:
            out["PSNR"] = sum(self.psnr) / len(self.psnr)
            out["SSIM"] = sum(self.ssim) / len(self.ssim)
        if self.lpips:
            out["LPIPS"] = sum(self.lpips) / len(self.lpips)
        if self.ssim3d:                                     # the mean over CLIPS, as run.py averages its per-video rows
            out["SSIM3D"] = sum(self.ssim3d) / len(self.ssim3d)
            out["SSIM2D"] = sum(self.ssim2d) / len(self.ssim2d)
        if len(self.fvd_ref) >= 2 and len(self.fvd_ref) == len(self.fvd_rec):
            out["FVD"] = frechet_distance(np.stack(self.fvd_ref), np.stack(self.fvd_rec))
        if self.motion:                                     # this project's own measure, not FVMD: the `fvdm` column stays blank
            s = motion_summary([c["ref"] for c in self.motion], self.motion)
            out["MotionEPE"] = s["motion_epe"]
            out["MotionMean"] = s["reconstruction"]["motion_mean"]
        return out

    def fvd_note(self) -> str:
        """what a driver prints after result() when it holds "FVD" (fvd_caption in brackets); the empty string otherwise"""
        if not (len(self.fvd_ref) >= 2 and len(self.fvd_ref) == len(self.fvd_rec)):
            return ""
        return f" (FVD: {fvd_caption(self.clips, self._fvd_synthetic())})"

    def _fvd_synthetic(self) -> bool:
        return self.fvd_model is not None and self.fvd_model.label == "synthetic"

    def save_csv(self, path: str) -> str:
        """one row per clip under the header of the fork's rebuttal/common_metrics_on_video_quality/run.py: `ssim` is ssim3d (its
        pytorch_msssim call), `psnr` the mean of the per-frame values (calculate_psnr.py's rule is scores_from_stats'), `lpips` the
        per-frame mean when the accumulator holds LPIPS weights and empty otherwise; `fvd` (run.py: the styleganv detector per video) and
        `fvdm` (a keypoint tracker) are out of scope and always empty"""
        import csv
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, mode="w", newline="") as f:
            w = csv.writer(f)
            w.writerow(METRICS_CSV_HEADER)
            w.writerows(self.csv_rows)
        return path

    def save(self, results_dir: str, root1: str, root2: str, timestamp: str = None) -> str:
        """the `FVD:` line, present only when result() has the key, carries the variant and the clip count beside the value"""
        res = self.result()
        if "FVD" in res:
            res["FVD"] = fvd_line(res["FVD"], self.clips, self._fvd_synthetic())
        if "MotionEPE" in res:
            s = motion_summary([c["ref"] for c in self.motion], self.motion)
            what = f"block {s['block']}, radius {s['radius']}, lam {s['lam']}; block matching on gray frames, this project's own measure, not FVMD"
            res["MotionEPE"] = f"{res['MotionEPE']} (px between the input's and the reconstruction's vector fields; {what})"
            res["MotionMean"] = f"{res['MotionMean']} (px/frame of the reconstructions; inputs {s['input']['motion_mean']})"
        return save_results(res, root1, root2, results_dir, timestamp)
