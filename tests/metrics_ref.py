"""float64 numpy restatement of the reference's per-frame scores (evaluation/compute_metrics.py:31-41 with skimage's
structural_similarity defaults: 7x7 uniform window, sample covariance, K1 0.01, K2 0.03, valid window positions only), formed from
exact integer box sums so it needs no skimage.  tests/test_metrics_cpu.py pins it to golden scores skimage itself produced; the GPU
tests then use it where no golden vector exists."""
import math

import numpy as np

WIN = 7


def quantise(x, rescale=True):
    """utils.file_utils.frames_uint8 on a float32 array: ((x + 1) / 2 if rescale), clamp(0, 1), * 255, truncate - each step in fp32."""
    x = np.asarray(x, dtype=np.float32)
    if rescale:
        x = (x + np.float32(1.0)) / np.float32(2.0)
    return (np.clip(x, np.float32(0.0), np.float32(1.0)) * np.float32(255.0)).astype(np.uint8)


def _box(a):
    """sum over every 7x7 window (valid positions) of an int64 [H, W] array, by summed-area table: exact"""
    s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    return s[WIN:, WIN:] - s[:-WIN, WIN:] - s[WIN:, :-WIN] + s[:-WIN, :-WIN]


def psnr(img1, img2):
    """uint8 [H, W, C] frames"""
    d = img1.astype(np.int64) - img2.astype(np.int64)
    mse = float((d * d).sum()) / float(d.size) / 255.0 ** 2
    return 100.0 if mse < 1.0e-10 else 20.0 * math.log10(1.0 / math.sqrt(mse))


def box_moments(x, y):
    """uint8 [H, W] planes -> the exact int64 7x7 box sums (sx, sy, sxx, syy, sxy), each [H-6, W-6]"""
    x, y = x.astype(np.int64), y.astype(np.int64)
    return _box(x), _box(y), _box(x * x), _box(y * y), _box(x * y)


def ssim_maps(img1, img2, R=None):
    """uint8 [H, W, C] frames -> the float64 SSIM map of every channel, [C, H-6, W-6]; data range R of img1's frame (all channels)
    unless given"""
    if img1.shape[0] < WIN or img1.shape[1] < WIN:
        raise ValueError("win_size exceeds image extent")
    R = float(int(img1.max()) - int(img1.min())) if R is None else float(R)
    C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    n = WIN * WIN
    out = np.zeros((img1.shape[2], img1.shape[0] - WIN + 1, img1.shape[1] - WIN + 1), dtype=np.float64)
    for c in range(img1.shape[2]):
        sx, sy, sxx, syy, sxy = box_moments(img1[..., c], img2[..., c])
        vx, vy, vxy = n * sxx - sx * sx, n * syy - sy * sy, n * sxy - sx * sy            # exact: the cancellation is in integers
        cov = float(n * (n - 1))
        a1 = 2.0 * (sx * sy) / float(n * n) + C1
        b1 = (sx * sx + sy * sy) / float(n * n) + C1
        a2 = 2.0 * vxy / cov + C2
        b2 = (vx + vy) / cov + C2
        out[c] = (a1 * a2) / (b1 * b2)
    return out


def ssim_map_sums(img1, img2, R=None):
    """per channel: sum of the SSIM map over the (H-6) x (W-6) window positions, float64 [C]; data range of img1's frame"""
    return np.array([m.sum() for m in ssim_maps(img1, img2, R)], dtype=np.float64)


def ssim(img1, img2):
    if img1.min() == img1.max() or img2.min() == img2.max():
        return 1.0
    npos = (img1.shape[0] - WIN + 1) * (img1.shape[1] - WIN + 1)
    return float(np.mean(ssim_map_sums(img1, img2) / npos))


def video_scores(ref, rec, rescale=True):
    """float arrays [C, T, H, W] -> (psnr [T], ssim [T]) over the common frames"""
    ref, rec = np.asarray(ref), np.asarray(rec)
    T = min(ref.shape[1], rec.shape[1])
    ps, ss = np.empty(T), np.empty(T)
    for t in range(T):
        f1 = quantise(ref[:, t], rescale).transpose(1, 2, 0)
        f2 = quantise(rec[:, t], rescale).transpose(1, 2, 0)
        ps[t], ss[t] = psnr(f1, f2), ssim(f1, f2)
    return ps, ss
