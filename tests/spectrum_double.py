"""fp32 CPU double of csrc/hv_spectrum.hip + the host rules of metrics.temporal_spectrum, in numpy: the same operands (the 8-bit gray
integers or the fp32 values, the pivot, the host-built twiddle table), re / im as fp32 fmaf chains over the frames, |X|^2 =
fl(fl(re^2) + fl(im^2)), |X| = fp32 sqrt, fp64 sums over series, division by the series count, mirroring.  The switches turn it into
the mutants tests/test_spectrum_cpu.py wants the bound to reject."""
import numpy as np

from hunyuanvideo_efficiency_amd import metrics
from tests import spectrum_ref

f32, f64 = np.float32, np.float64


def table_columns(T, table=None):
    """(cos [T, T // 2], sin [T, T // 2]) fp32, read out of the kernel's table layout"""
    tab = (metrics.spectrum_twiddles(T).numpy() if table is None else table)
    nb = T // 2
    ncol = tab.shape[1] // 64
    t4 = tab.reshape(tab.shape[0], ncol, 2, 32)
    return t4[:T, :, 0].reshape(T, -1)[:, :nb], t4[:T, :, 1].reshape(T, -1)[:, :nb]


def unreduced_fp32_twiddles(T):
    """the mutant table: the angle 2 pi k t / T formed in fp32 without reducing k t mod T"""
    k = np.arange(1, T // 2 + 1, dtype=f32)[None, :]
    t = np.arange(T, dtype=f32)[:, None]
    ang = f32(2.0) * f32(np.pi) * k * t / f32(T)
    return np.cos(ang.astype(f64)).astype(f32), np.sin(ang.astype(f64)).astype(f32)


def _fma(acc, a, b):
    """fl32(acc + a * b) with the product exact (it fits float64)"""
    return (acc.astype(f64) + a.astype(f64) * b.astype(f64)).astype(f32)


def _order(T, order):
    if order == "frames":                    # the kernel: one chain in frame order
        return np.arange(T)
    if order == "reversed":
        return np.arange(T)[::-1]
    if order == "rotated":                   # a chain that starts in the middle of the clip
        return np.roll(np.arange(T), T // 2)
    raise ValueError(order)


def series_spectrum(signal, gray, order="frames", pivot=True, twiddles=None, re_only=False):
    """signal [T, N] (integers, or fp32 values held in float64) -> fp32 per-series (|X| [K, N], |X|^2 [K, N]), K = T // 2 + 1"""
    signal = np.asarray(signal)
    T, N = signal.shape
    x = signal.astype(f32)                                       # exact: bytes, or fp32 values
    d = (x - x[:1]).astype(f32) if pivot else x                 # one fp32 rounding in raw mode, none for integers
    cos, sin = table_columns(T) if twiddles is None else twiddles
    nb = T // 2
    re, im = np.zeros((N, nb), f32), np.zeros((N, nb), f32)
    for t in _order(T, order):
        re = _fma(re, d[t][:, None], cos[t][None, :])
        im = _fma(im, d[t][:, None], sin[t][None, :])
    pw = ((re * re).astype(f32) + (np.zeros_like(im) if re_only else (im * im).astype(f32))).astype(f32)
    mag = np.sqrt(pw).astype(f32)
    if gray:
        dc = signal.astype(np.int64).sum(axis=0).astype(f64)     # exact integers
        dc_mag, dc_pow = np.abs(dc), dc * dc
    else:
        s = np.zeros(N, f32)
        for t in range(T):                                       # the unshifted fp32 chain in frame order
            s = (s + x[t]).astype(f32)
        dc_mag, dc_pow = np.abs(s).astype(f64), (s * s).astype(f32).astype(f64)
    return (np.concatenate([dc_mag[None], mag.T.astype(f64)]), np.concatenate([dc_pow[None], pw.T.astype(f64)]))


def temporal_spectrum(x, mode="gray", rescale=True, luma=spectrum_ref.GRAY_LUMA, order="frames", pivot=True, twiddles=None,
                      re_only=False, drop_last_frame=False, padded_count=False, swap_rb=False, mirror_off_by_one=False, double_nyquist=False):
    """the double of metrics.temporal_spectrum on a float array [C, T, H, W] -> {"magnitude" [T], "power" [T]}"""
    x = np.asarray(x, dtype=f32)
    if swap_rb:
        x = x[::-1]
    gray = mode == "gray"
    signal = spectrum_ref.gray_series(x, rescale, luma) if gray else spectrum_ref.raw_series(x)
    T, N = signal.shape
    work = signal.copy()
    if drop_last_frame:
        work[-1] = work[0]                                       # d = 0: the frame adds nothing to the bins k >= 1
    mag, pw = series_spectrum(work, gray, order, pivot, twiddles, re_only)
    count = -(-N // 256) * 256 if padded_count else N
    out = {}
    for name, v in (("magnitude", mag), ("power", pw)):
        half = v.sum(axis=1) / float(count)
        if double_nyquist and T % 2 == 0:
            half[-1] *= 2.0
        if mirror_off_by_one:                                    # bin T - k takes bin k - 1
            full = np.concatenate([half, half[:(T + 1) // 2 - 1][::-1]])
        else:
            full = metrics.mirror_spectrum(half, T)
        out[name] = full
    return out
