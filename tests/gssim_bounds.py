"""Error bound of the Gaussian-window SSIM kernel (csrc/hv_gssim.hip) against tests/gssim_ref.py, derived from the arithmetic
include/hv_gssim.h states, and `kernel_double`, a stepwise numpy restatement of that arithmetic which tests/test_gssim_cpu.py feeds to
the very assertions tests/test_gpu_gssim.py uses (`check_sums`).  In the conventions of tests/metrics_bounds.py and tests/tinterp_bounds.py.

u = 2^-53.  Both sides are fp64; neither is exact, so the bound is the sum of the two sides' errors against the real-number value.

Fields.  A 1-D pass is an 11-term chain of non-negative terms, acc = w0 v0, acc = fma(wk, vk, acc): term k meets at most 11 roundings
(its own, where the product is rounded separately as in numpy, and the additions after it), so the pass returns sum wk vk (1 + theta_k),
|theta_k| <= 12 u (11 u and the second-order terms).  All weights and values are >= 0, so the relative error carries through the next
pass: after T, H and W a filtered field F is off by at most ((1 + 12 u)^3 - 1) F < 37 u F.  The kernel's inputs are exact (integers, and
products of integers below 2^17); the reference divides the codes by 255 and squares them first, three more roundings.
    EPS_FIELD = 40 u, relative, for either side, for each of m1, m2, e11, e22, e12 (the filtered x, y, xx, yy, xy).
Map.  With e = EPS_FIELD, in any one unit (the map does not change when codes, C1 and C2 are scaled together):
    m_i m_j rounded            off by (2 e + u) m_i m_j
    s_ij = e_ij - m_i m_j      off by  d_ij = e e_ij + (2 e + u) m_i m_j + u |s_ij|                      <- the cancellation: e_ij ~ 65025
    lum = (2 m1 m2 + C1) / (m1^2 + m2^2 + C1) <= 1:  numerator off by 2 (2 e + u) m1 m2 + u N, denominator by (2 e + u)(m1^2 + m2^2) + 2 u D,
          so lum by ((2 e + u)(2 m1 m2 + m1^2 + m2^2) + 3 u D) / D + u <= 4 e + 6 u
    cs = (2 s12 + C2) / (s1 + s2 + C2), |cs| <= 1 (Cauchy-Schwarz; the weights sum to at most 1 + 2 u):  off by
          (2 d12 + d11 + d22) / (s1 + s2 + C2) + 4 u
    map = lum cs rounded, |lum|, |cs| <= 1:  off by  MAP(pos) = (2 d12 + d11 + d22) / (s1 + s2 + C2) + 4 e + 11 u.
    The reference's rounded C1, C2 and its other association (calculate_ssim.py multiplies numerators and denominators first) move a
    value by 2 u more.  Second-order terms are below 2^-40 of the bound; the bound carries the factor 1 + 2^-30.
    per map value   |kernel - reference| <= 2 (MAP(pos) + 2 u) (1 + 2^-30)                 (both sides)
Sums.  The reference's sums are correctly rounded (math.fsum): u |sum|.  The kernel adds at most two values a thread, folds 64 lanes in six
steps, four waves in three and the tiles of a frame in order: a value meets at most 11 + ntiles additions, each rounding a partial sum of
magnitude <= npos (|map| <= 1):
    per sum         |kernel - reference| <= sum over positions of the map bound + (12 + ntiles) u npos.
`bounds(..., u=2^-24)` gives the same expressions for an fp32 evaluation; the flat-bright condition of the issue (test_gssim_cpu) holds
for fp64 with five orders of magnitude to spare and fails there."""
import math

import numpy as np

from hunyuanvideo_efficiency_amd import _abi
from tests import gssim_ref as ref

U = 2.0 ** -53
WIN = _abi.GSSIM_MACROS["HV_GSSIM_WIN"]
TILE_H, TILE_W = _abi.GSSIM_MACROS["HV_GSSIM_TILE_H"], _abi.GSSIM_MACROS["HV_GSSIM_TILE_W"]
FIELD_ROUNDINGS = 40.0
KC1, KC2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2        # the kernel's constants, in code units


def ntiles(H, W):
    return -(-(H - WIN + 1) // TILE_H) * -(-(W - WIN + 1) // TILE_W)


def map_bound(a, b, w, temporal, u=U):
    """per map value, [C,To,H-10,W-10]: the bound on |kernel - reference| derived above, from the reference's own fields"""
    e = FIELD_ROUNDINGS * u
    X, Y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    axes = (1, 2, 3) if temporal else (2, 3)
    m1, m2 = ref.filter_valid(X, w, axes), ref.filter_valid(Y, w, axes)
    e11, e22, e12 = ref.filter_valid(X * X, w, axes), ref.filter_valid(Y * Y, w, axes), ref.filter_valid(X * Y, w, axes)
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2

    def d(eij, mm, s):
        return e * eij + (2 * e + u) * mm + u * np.abs(s)
    one = (2 * d(e12, m1 * m2, s12) + d(e11, m1 * m1, s1) + d(e22, m2 * m2, s2)) / (np.maximum(s1 + s2, 0.0) + KC2) + 4 * e + 11 * u
    return 2.0 * (one + 2 * u) * (1.0 + 2.0 ** -30)


def sum_bound(a, b, w, temporal, u=U):
    """[To][C]: the bound on |ssim_sum - reference sum|"""
    mb = map_bound(a, b, w, temporal, u)
    C, To, h, wd = mb.shape
    return mb.reshape(C, To, -1).sum(axis=2).T + (12 + ntiles(h + WIN - 1, wd + WIN - 1)) * u * (h * wd)


def chain(x, w, ax):
    """one 1-D pass as the header orders it: acc = w[0] v[0], then acc = acc + w[k] v[k] for k = 1 .. 10 (the product rounded on its own:
    numpy has no fma; the bound counts that rounding)"""
    n = x.shape[ax]
    acc = w[0] * np.take(x, np.arange(0, n - WIN + 1), axis=ax)
    for k in range(1, WIN):
        acc = acc + w[k] * np.take(x, np.arange(k, n - WIN + 1 + k), axis=ax)
    return acc


def kernel_double(a, b, w, temporal):
    """codes uint8 [C,T,H,W] -> [To][C] sums the way the kernel forms them: code units, passes T, H, W, the header's map, tile partials
    (rows of a tile in order) folded in tile order"""
    X, Y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    f = [X, Y, X * X, Y * Y, X * Y]
    for ax in ((1, 2, 3) if temporal else (2, 3)):
        f = [chain(v, w, ax) for v in f]
    m1, m2, e11, e22, e12 = f
    m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
    s1, s2, s12 = e11 - m11, e22 - m22, e12 - m12
    m = (((2.0 * m12) + KC1) / ((m11 + m22) + KC1)) * (((2.0 * s12) + KC2) / ((s1 + s2) + KC2))
    C, To, h, wd = m.shape
    out = np.zeros((To, C))
    for t in range(To):
        for c in range(C):
            total = None
            for y0 in range(0, h, TILE_H):
                for x0 in range(0, wd, TILE_W):
                    part = float(np.sum(m[c, t, y0:y0 + TILE_H, x0:x0 + TILE_W]))
                    total = part if total is None else total + part
            out[t, c] = total
    return out


def check_sums(got, a, b, w, temporal, tag=""):
    """the assertion of the GPU test: every [To][C] sum within its bound of the reference; returns the largest error / bound"""
    want = ref.sums(a, b, w, temporal)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: non-finite sums"
    bound = sum_bound(a, b, w, temporal)
    ratio = np.abs(got - want) / bound
    assert (ratio <= 1.0).all(), f"{tag}: |sum - reference| is {ratio.max():.3g} of the bound at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return float(ratio.max())


def flat_pair(T=13, H=24, W=24, C=1):
    """the issue's sensitivity input: a flat clip of code 250 and a copy with one pixel, in the middle frame, at 251"""
    a = np.full((C, T, H, W), 250, dtype=np.uint8)
    b = a.copy()
    b[0, T // 2, H // 2, W // 2] = 251
    return a, b


def rand_codes(shape, seed, lo=0, hi=255):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape, dtype=np.int64).astype(np.uint8)


def noisy_codes(shape, seed, amp=9):
    a = rand_codes(shape, seed)
    d = np.random.default_rng(seed + 1).integers(-amp, amp + 1, size=shape)
    return a, np.clip(a.astype(np.int64) + d, 0, 255).astype(np.uint8)
