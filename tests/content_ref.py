"""numpy restatement (int64 counts, float64 everything else) of the content statistics of csrc/hv_content.hip and the host rules of
metrics.content_entropy / content_bucket.  The 8-bit frame and the gray byte are the ones the spectrum's reference uses
(tests/spectrum_ref.gray_series on tests/metrics_ref's quantiser rule: utils.file_utils.frames_uint8, then the integer luma).

The measure is this project's own definition (the fork publishes bucket names and edges only): inter-frame entropy = Shannon entropy, in
bits, of the histogram of gray[t + 1] - gray[t], averaged over the frame pairs of a clip."""
import numpy as np

from tests import metrics_ref
from tests.spectrum_ref import GRAY_LUMA, gray_series

INTER_BINS = 511
EDGES = (2.0, 4.0, 6.0)
LABELS = ("Very_Low_InterEntropy_lt2", "Low_InterEntropy_2-4", "Medium_InterEntropy_4-6", "High_InterEntropy_gt6")
DEFINITION = ("entropy of the 8-bit gray frame difference histogram, bits; this project's definition, the fork publishes only the bucket "
              "names")
ENTROPY_TOL = 1e-10     # bits: at most 1024 terms c log2(c) / N <= 31, each a few ulp of 2^-52 -> below 1e-11; ten times that


def gray_frames(x, rescale=True, luma=GRAY_LUMA):
    """float array [3, T, H, W] -> int64 [T, H * W] gray bytes"""
    g = gray_series(x, rescale, luma)
    assert g.min() >= 0 and g.max() <= 255
    return g


def gray_of_bytes(rgb, luma=GRAY_LUMA):
    """the integer luma of quantised bytes [..., 3] (for the known-answer cases that start from bytes)"""
    wr, wg, wb, rnd, shift = luma
    rgb = np.asarray(rgb).astype(np.int64)
    return (wr * rgb[..., 0] + wg * rgb[..., 1] + wb * rgb[..., 2] + rnd) >> shift


def quantised_gray(values, rescale=True, luma=GRAY_LUMA):
    """the gray byte of a pixel whose three channels all hold `values` (any shape): metrics_ref.quantise, then the luma"""
    q = metrics_ref.quantise(np.asarray(values, dtype=np.float32), rescale).astype(np.int64)
    return gray_of_bytes(np.stack([q, q, q], axis=-1), luma)


def histograms_of_gray(g):
    """g int64 [T, N] -> (intra int64 [T, 256], inter int64 [T - 1, 511])"""
    g = np.asarray(g).astype(np.int64)
    T = g.shape[0]
    intra = np.stack([np.bincount(g[t], minlength=256) for t in range(T)]).astype(np.int64)
    inter = np.zeros((T - 1, INTER_BINS), dtype=np.int64)
    for t in range(T - 1):
        inter[t] = np.bincount(g[t + 1] - g[t] + 255, minlength=INTER_BINS)
    return intra, inter


def histograms(x, rescale=True, luma=GRAY_LUMA):
    return histograms_of_gray(gray_frames(x, rescale, luma))


def row_stats(counts, origin):
    """counts int [rows, bins] -> float64 [rows, 3]: entropy in bits (log2 N - sum c log2 c / N; 0 for an empty row), and the exact
    integer moments sum c v, sum c v^2 with v = bin - origin, as floats"""
    counts = np.asarray(counts).astype(np.int64).reshape(-1, np.asarray(counts).shape[-1])
    out = np.zeros((counts.shape[0], 3), dtype=np.float64)
    v = np.arange(counts.shape[1], dtype=np.int64) - origin
    for r, c in enumerate(counts):
        n = int(c.sum())
        if n:
            nz = c[c > 0].astype(np.float64)
            out[r, 0] = max(np.log2(float(n)) - float((nz * np.log2(nz)).sum()) / float(n), 0.0)
        s1, s2 = int((c * v).sum()), int((c * v * v).sum())
        assert abs(s1) < 2 ** 53 and s2 < 2 ** 53
        out[r, 1], out[r, 2] = float(s1), float(s2)
    return out


def content_entropy(x, rescale=True, luma=GRAY_LUMA):
    """the double of metrics.content_entropy on a float array [3, T, H, W]"""
    g = gray_frames(x, rescale, luma)
    return content_of_gray(g)


def content_of_gray(g):
    g = np.asarray(g).astype(np.int64)
    T, n = g.shape
    intra, inter = histograms_of_gray(g)
    si, sp = row_stats(intra, 0), row_stats(inter, 255)
    d = {"inter_entropy": None, "intra_entropy": float(si[:, 0].mean()), "intra_entropy_frames": si[:, 0].tolist(),
         "inter_entropy_pairs": sp[:, 0].tolist(), "mean_abs_diff": None, "ti": None, "frames": int(T), "definition": DEFINITION}
    if T > 1:
        diff = g[1:] - g[:-1]
        d["inter_entropy"] = float(sp[:, 0].mean())
        d["mean_abs_diff"] = float(np.mean([int(np.abs(r).sum()) / n for r in diff]))
        # ITU-T P.910: max over time of the spatial standard deviation; the variance from exact integers, rounded once
        d["ti"] = float(np.sqrt(max((n * int((r * r).sum()) - int(r.sum()) ** 2) / float(n * n) for r in diff)))
    return d


def bucket(value, edges=EDGES, labels=LABELS):
    """half-open [lo, hi): a value on an edge belongs to the bucket above it; None has no bucket"""
    if value is None:
        return None
    return labels[int(np.searchsorted(np.asarray(edges, dtype=np.float64), float(value), side="right"))]


def measure(dataset, n):
    """the numpy stand-in for tools/bucket_clips.measure_on_gpu"""
    return [content_entropy(np.asarray(dataset[i][0], dtype=np.float32)) for i in range(n)]
