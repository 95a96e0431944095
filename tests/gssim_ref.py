"""float64 numpy restatement of the two Gaussian-window SSIM scores of the fork's rebuttal/common_metrics_on_video_quality, from 8-bit
codes.  Written from run.py:61-68 (pytorch_msssim.ssim(v1, v2, data_range=1.0, size_average=True) on [B,C,T,H,W]), from calculate_ssim.py
beside it, and from the published definition of pytorch_msssim.ssim - not from the kernel:

  pytorch_msssim   win = _fspecial_gauss_1d(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)) in fp32, divided by its fp32 sum.  gaussian_filter
                   applies it along every spatial axis of the input in turn (T, H, W for a 5-D input) with a valid, grouped convolution;
                   an axis shorter than the window is skipped with a warning.  mu = filter(X), sigma = filter(X X) - mu mu (compensation
                   1.0), cs = (2 sigma12 + C2) / (sigma1 + sigma2 + C2), map = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) cs, C1 = (0.01
                   data_range)^2, C2 = (0.03 data_range)^2; the map is averaged per channel, then over channels (size_average).  No
                   constant-frame case, no per-frame data range.
  calculate_ssim   per frame and channel, float64: window = outer(k, k), k = cv2.getGaussianKernel(11, 1.5) (the same formula in double,
                   normalised in double); filter2D cropped to the valid positions; map = ((2 mu1 mu2 + C1)(2 sigma12 + C2)) /
                   ((mu1^2 + mu2^2 + C1)(sigma1 + sigma2 + C2)); the mean over the map, then over channels, then over frames.  Its
                   callers hand it frames in [0, 1] (C1, C2 are 0.01^2, 0.03^2).

Neither pytorch_msssim nor cv2 is part of this environment; tests/test_gssim_cpu.py anchors this file against a torch float64 grouped
convolution, against scipy.ndimage.correlate1d and against known answers.  Sums over a map are math.fsum: correctly rounded."""
import math
import warnings

import numpy as np

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(form):
    """the 11 weights as float64: form "fp32" - pytorch_msssim._fspecial_gauss_1d(11, 1.5), torch operations in fp32 as that function
    performs them (coords = arange - 5; g = exp(-coords^2 / (2 sigma^2)); g /= g.sum()), widened; "fp64" - the formula in double,
    normalised in double (cv2.getGaussianKernel)"""
    if form == "fp32":
        import torch
        coords = torch.arange(WIN, dtype=torch.float)
        coords -= WIN // 2
        g = torch.exp(-(coords ** 2) / (2 * SIGMA ** 2))
        g /= g.sum()
        return g.numpy().astype(np.float64)
    assert form == "fp64"
    g = np.exp(-((np.arange(WIN, dtype=np.float64) - WIN // 2) ** 2) / (2 * SIGMA ** 2))
    return g / g.sum()


def filter_valid(x, w, axes):
    """valid correlation of x with the 1-D window w along each of `axes` in turn; an axis shorter than the window is skipped"""
    for ax in axes:
        n = x.shape[ax]
        if n < WIN:
            continue
        acc = None
        for k in range(WIN):
            term = w[k] * np.take(x, np.arange(k, n - WIN + 1 + k), axis=ax)
            acc = term if acc is None else acc + term
        x = acc
    return x


def fields(a, b, w, axes):
    """codes uint8 [C,T,H,W] -> (mu1, mu2, sigma1, sigma2, sigma12) of the frames / 255"""
    X, Y = np.asarray(a, dtype=np.float64) / 255.0, np.asarray(b, dtype=np.float64) / 255.0
    mu1, mu2 = filter_valid(X, w, axes), filter_valid(Y, w, axes)
    s1 = filter_valid(X * X, w, axes) - mu1 * mu1
    s2 = filter_valid(Y * Y, w, axes) - mu2 * mu2
    s12 = filter_valid(X * Y, w, axes) - mu1 * mu2
    return mu1, mu2, s1, s2, s12


def ssim_map(a, b, w, temporal):
    """the pytorch_msssim form of the map, [C,To,H-10,W-10]; temporal: the window runs along T too"""
    mu1, mu2, s1, s2, s12 = fields(a, b, w, (1, 2, 3) if temporal else (2, 3))
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs


def map_sums(m):
    """[C,To,h,w] -> float64 [To][C], each the correctly rounded sum of a map"""
    C, To = m.shape[:2]
    return np.array([[math.fsum(m[c, t].ravel().tolist()) for c in range(C)] for t in range(To)], dtype=np.float64).reshape(To, C)


def sums(a, b, w, temporal):
    """what hv_gaussian_ssim returns: [To][C] sums of the map"""
    if temporal and np.asarray(a).shape[1] < WIN:
        raise ValueError("the temporal window needs 11 frames")
    return map_sums(ssim_map(a, b, w, temporal))


def ssim3d(a, b):
    """the run.py score of one video: fp32-form window over T, H, W (T < 11: over H, W, with pytorch_msssim's warning); the mean of the map
    per channel, then over channels"""
    a, b = np.asarray(a), np.asarray(b)
    temporal = a.shape[1] >= WIN
    if not temporal:
        warnings.warn(f"Skipping Gaussian Smoothing at dimension 2 for input: {a.shape} and win size: {WIN}")
    m = ssim_map(a, b, window("fp32"), temporal)
    return float(np.mean([math.fsum(m[c].ravel().tolist()) / m[c].size for c in range(m.shape[0])]))


def ssim2d_frames(a, b):
    """the calculate_ssim.py score per frame: fp64-form window, the product form of the map, mean over positions, then over channels"""
    a, b = np.asarray(a), np.asarray(b)
    mu1, mu2, s1, s2, s12 = fields(a, b, window("fp64"), (2, 3))
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    C, T = m.shape[:2]
    return np.array([np.mean([math.fsum(m[c, t].ravel().tolist()) / m[c, t].size for c in range(C)]) for t in range(T)])


def ssim2d(a, b):
    return float(np.mean(ssim2d_frames(a, b)))
