"""float64 numpy restatement of the fork's temporal spectra (theory_analysis.ipynb cells 2, 4, 5) and the error bound of the device
kernel (csrc/hv_spectrum.hip) against it.

The reference (cell 2 / the first half of cells 4, 5): every frame goes through cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY), the frames are
stacked to `signal` [T, H * W], and the plotted curve is `np.abs(np.fft.fft(signal, axis=0)).mean(axis=1)`.  The second half of cells
4, 5 does the same over `latent_dist.mean.permute(0, 1, 3, 4, 2).reshape(-1, T_lat)`: one series per (channel, h, w).  Here the 8-bit
frame is the one `utils.file_utils.frames_uint8` writes, and the gray byte is the integer rule (wr R + wg G + wb B + round) >> shift
with GRAY_LUMA - OpenCV's 8-bit BGR2GRAY as restated from its documentation (0.299, 0.587, 0.114 in 15 fractional bits, rounded to
nearest).  cv2 is not part of this environment: THE RULE IS A RESTATEMENT AND IS NOT PINNED against OpenCV.

Error bound (the tests/error_bounds.py convention: 4 standard deviations of an fp32 chain whose roundings are independent).  The kernel
transforms d_t = x_t - x_0 (exact integers in gray mode; one fp32 rounding each in raw mode) with fp32 twiddles rounded once from
float64, one fp32 chain of T terms for re and one for im, then |X|^2 = fl(fl(re^2) + fl(im^2)) and |X| = sqrtf.  Per series and bin
k >= 1

    | |X| - |X64| |      <=  delta_k + 2^-23 |X64|,      delta_k = 4 sqrt(2 T) 2^-24 max(||d||_2, P_k)
    | |X|^2 - |X64|^2 |  <=  2 |X64| delta_k + delta_k^2,    P_k = max_j |sum_{t <= j} d_t exp(-2 pi i k t / T)|

The first-order error of a chain is sum_j eps_j s_j over its partial sums s_j, |eps_j| <= 2^-24: a spread of at most
2^-24 sqrt(T) max_j |s_j| per component (the twiddles' 2^-25 relative roundings and, in raw mode, the 2^-24 relative rounding of d_t
are sums of T terms of size 2^-24 |d_t| and fit under the ||d||_2 term; 2^-23 |X64| is the squaring, adding and sqrtf roundings).
For zero-mean random data the partial sums are a random walk of size ||d||_2, the only term the bound had at first.  P_k is the term
that form misses: the pivot x_0 leaves d an offset x_0 - mean, and a trend does the same, whose partial sums in a low bin reach
|offset| T / (pi k) - T rather than sqrt(T) - although they cancel in the final X_k.  Without P_k the fp32 CPU double reached 0.74 of
the bound in the kernel's frame order at T = 600 and 1.10 when the chain starts in the middle of a ramp; with it every order stays below
0.3 (tests/test_spectrum_cpu.py has the table).  P_k is taken in frame order, the kernel's; a reversed chain or one that starts
mid-clip has partial sums that are differences of two of these prefix sums, at most 2 P_k, which the factor 4 covers.
Gray-mode bin 0 is exact.  Raw-mode bin 0 is an fp32 chain of the UNSHIFTED values in frame order: the same form with
||x||_2 + max_j |sum_{t <= j} x_t| (the order of this chain is fixed by the kernel's contract; a -1 .. 1 ramp of 129 samples reaches
2.6 x the ||x||_2 bound alone, 0.73 x this one).  The bound on a mean over series is the mean of the bounds."""
import numpy as np
import torch

from hunyuanvideo_efficiency_amd.utils.file_utils import frames_uint8

GRAY_LUMA = (9798, 19235, 3735, 1 << 14, 15)      # wr, wg, wb, round, shift
EPS32 = 2.0 ** -24
C = 4.0


def gray_series(x, rescale=True, luma=GRAY_LUMA):
    """float array [3, T, H, W] -> int64 [T, H * W]: the gray byte of every pixel of every 8-bit frame"""
    x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    frames = np.stack(frames_uint8(x[None], rescale=rescale)).astype(np.int64)          # [T, H, W, 3]
    wr, wg, wb, rnd, shift = luma
    y = (wr * frames[..., 0] + wg * frames[..., 1] + wb * frames[..., 2] + rnd) >> shift
    return y.reshape(y.shape[0], -1)


def raw_series(x):
    """float array [C, T, H, W] -> float64 [T, C * H * W] holding the fp32 values: cell 4's permute + reshape, transposed"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1)


class Spectrum:
    """reference and bound of one [T, N] signal; `gray`: integer series (bin 0 exact)"""

    def __init__(self, signal, gray):
        signal = np.asarray(signal)
        self.T, self.N = signal.shape
        T = self.T
        s64 = signal.astype(np.float64)
        d = s64 - s64[:1]
        X = np.abs(np.fft.fft(s64, axis=0))                                             # [T, N], cells 2 / 4
        X[1:] = np.abs(np.fft.fft(d, axis=0))[1:]      # the same numbers without the float64 leakage of a large DC term into them
        P = X * X
        delta = C * np.sqrt(2.0 * T) * EPS32 * np.maximum(np.sqrt((d * d).sum(axis=0))[None], prefix_max(d))     # [T, N]
        mag_b = delta + 2.0 ** -23 * X
        pow_b = 2.0 * X * delta + delta ** 2
        if gray:
            tot = [int(v) for v in signal.astype(np.int64).sum(axis=0)]
            X[0] = np.abs(np.array(tot, dtype=np.float64))
            P[0] = np.array([float(v * v) for v in tot])
            self.dc_sums = (sum(abs(v) for v in tot), sum(v * v for v in tot))          # exact python integers
            mag_b[0] = pow_b[0] = 0.0
        else:
            d0 = C * np.sqrt(2.0 * T) * EPS32 * (np.sqrt((s64 * s64).sum(axis=0)) + np.abs(np.cumsum(s64, axis=0)).max(axis=0))
            mag_b[0] = d0 + 2.0 ** -23 * X[0]
            pow_b[0] = 2.0 * X[0] * d0 + d0 ** 2 + 2.0 ** -23 * P[0]
        self.series_mag, self.series_pow, self.series_mag_bound, self.series_pow_bound = X, P, mag_b, pow_b
        if gray:
            self.magnitude = np.concatenate([[self.dc_sums[0] / self.N], X[1:].mean(axis=1)])
            self.power = np.concatenate([[self.dc_sums[1] / self.N], P[1:].mean(axis=1)])
        else:
            self.magnitude, self.power = X.mean(axis=1), P.mean(axis=1)
        self.mag_bound, self.pow_bound = mag_b.mean(axis=1), pow_b.mean(axis=1)

    def ratios(self, magnitude, power):
        """largest |got - ref| / bound of full-length mean spectra over the bins k >= 1 and the error of bin 0 over its bound (bin 0 of an
        integer signal has bound 0: its ratio is 0 when exact, inf otherwise) -> (mag ratio, pow ratio)"""
        out = []
        for got, ref, b in ((magnitude, self.magnitude, self.mag_bound), (power, self.power, self.pow_bound)):
            got = np.asarray(got, dtype=np.float64)
            assert got.shape == ref.shape, (got.shape, ref.shape)
            err = np.abs(got - ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(err == 0.0, 0.0, err / b)
            out.append(float(np.max(np.where(np.isfinite(got), r, np.inf))))
        return tuple(out)


def prefix_max(d):
    """d [T, N] float64 -> [T, N]: row k holds max_j |sum_{t <= j} d_t exp(-2 pi i k t / T)|, the largest partial sum of bin k's chain
    in frame order (row 0 is unused and zero; row T - k equals row k)"""
    T, N = d.shape
    out = np.zeros((T, N))
    nb = T // 2
    step = max(1, (1 << 22) // max(T * N, 1))
    t = np.arange(T, dtype=np.int64)[:, None]
    for k0 in range(1, nb + 1, step):
        k = np.arange(k0, min(k0 + step, nb + 1), dtype=np.int64)[None, :]
        e = np.exp(-2j * np.pi * ((t * k) % T).astype(np.float64) / T)                  # [T, kc]
        out[k[0]] = np.abs(np.cumsum(d[:, None, :] * e[:, :, None], axis=0)).max(axis=0)
    out[T - nb:] = out[1:nb + 1][::-1]
    return out


def parseval_rhs(signal):
    """T sum_t d_t^2 - (sum_t d_t)^2 summed over the series of an INTEGER signal [T, N], d = x - x_0, in exact python integers:
    what sum_{k >= 1} |X_k|^2 over the full mirrored spectrum must equal, summed over series"""
    s = np.asarray(signal).astype(np.int64)
    d = s - s[:1]
    T = s.shape[0]
    return T * int((d * d).sum()) - sum(int(v) ** 2 for v in d.sum(axis=0))
