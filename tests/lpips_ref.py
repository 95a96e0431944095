"""Float64 torch-CPU restatement of the reference's lpips.LPIPS(net="alex") in its defaults (version 0.1, lpips=True, spatial=False,
eval mode), as the fork's evaluation/compute_metrics.py:43-62 calls it per frame.  Neither torchvision nor the `lpips` package is
available, so this file - not a package - is what the GPU path is compared with.

  * input (compute_metrics.py:44-60): x = float32(q / 255.0) * 2 - 1 on the 8-bit frame q, the division in float64, the rest in fp32;
    then the ScalingLayer (rebuttal/common_metrics_on_video_quality/lpips/lpips.py:147-154) (x - shift) / scale, fp32.  Both are the
    package's `metrics.lpips_lut`, built from those very torch operations (tests/test_lpips_cpu.py checks it entry by entry); from
    there on this restatement runs in `dtype` (float64; float32 to measure what fp32 arithmetic alone costs).
  * trunk (lpips/pretrained_networks.py:56-94 over torchvision alexnet features[0:12]): conv 3->64 k11 s4 p2, ReLU (tap 1), maxpool
    3/2, conv 64->192 k5 p2, ReLU (tap 2), maxpool 3/2, conv 192->384 k3 p1, ReLU (tap 3), conv 384->256 k3 p1, ReLU (tap 4),
    conv 256->256 k3 p1, ReLU (tap 5).
  * distance (lpips.py:122-139, lpips/__init__.py:13-15): n = f / (sqrt(sum_c f^2) + 1e-10); d_l = mean over pixels of
    sum_c lin_l[c] (n0 - n1)^2 (the NetLinLayer 1x1 conv, lpips.py:157-167, then spatial_average); LPIPS = sum_l d_l."""
import numpy as np
import torch
import torch.nn.functional as F

from hunyuanvideo_efficiency_amd import metrics
from tests import metrics_ref

POOL_AFTER = (0, 1)            # maxpool 3/2 behind taps 1 and 2


def scaled_input(q, dtype=torch.float64):
    """uint8 frame [H, W, 3] (numpy) -> network input [1, 3, H, W]: the fp32 LUT value of every byte, exact in either dtype"""
    lut = metrics.lpips_lut()
    qi = torch.from_numpy(np.ascontiguousarray(q)).long()
    x = torch.stack([lut[c][qi[..., c]] for c in range(3)])
    return x[None].to(dtype)


def taps(x, model, dtype=torch.float64):
    """network input [N, 3, H, W] -> the five tap feature maps [N, C_l, h_l, w_l]"""
    out = []
    for i, ((w, b), (_, _, _, _, stride, pad)) in enumerate(zip(model.convs, metrics.LPIPS_CONVS)):
        x = F.relu(F.conv2d(x, w.to(dtype), b.to(dtype), stride=stride, padding=pad))
        out.append(x)
        if i in POOL_AFTER:
            x = F.max_pool2d(x, kernel_size=3, stride=2)
    return out


def layer_distance(f0, f1, lin):
    """[N, C, h, w] features of both images, lin [C] -> per-image d_l [N]"""
    n0 = f0 / (torch.sqrt(torch.sum(f0 ** 2, dim=1, keepdim=True)) + 1e-10)
    n1 = f1 / (torch.sqrt(torch.sum(f1 ** 2, dim=1, keepdim=True)) + 1e-10)
    d = (n0 - n1) ** 2
    return (d * lin.to(d.dtype).reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def frame(q0, q1, model, dtype=torch.float64):
    """two uint8 frames [H, W, 3] -> (taps of q0, taps of q1, per-layer values [5], total)"""
    t0, t1 = taps(scaled_input(q0, dtype), model, dtype), taps(scaled_input(q1, dtype), model, dtype)
    layers = np.array([float(layer_distance(a, b, lin)[0]) for a, b, lin in zip(t0, t1, model.lins)], dtype=np.float64)
    return t0, t1, layers, float(layers.sum())


def video(ref, rec, model, rescale=True, dtype=torch.float64):
    """float arrays [3, T, H, W] -> (LPIPS [T], per-layer values [T, 5]) over the common frames, on the frames_uint8 bytes"""
    ref, rec = np.asarray(ref), np.asarray(rec)
    T = min(ref.shape[1], rec.shape[1])
    q0, q1 = metrics_ref.quantise(ref[:, :T], rescale), metrics_ref.quantise(rec[:, :T], rescale)
    total, layers = np.empty(T), np.empty((T, 5))
    for t in range(T):
        _, _, layers[t], total[t] = frame(q0[:, t].transpose(1, 2, 0), q1[:, t].transpose(1, 2, 0), model, dtype)
    return total, layers
