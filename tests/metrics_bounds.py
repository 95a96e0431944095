"""Case tables, input sets and references of the scoring-kernel edge tests (tests/test_gpu_quantiser.py, tests/test_gpu_metrics_edges.py;
what the references themselves satisfy: tests/test_metrics_bounds_cpu.py).  Everything here is host numpy; the fp64 SSIM and the
fp32-stepwise quantiser are those of tests/metrics_ref.py.

Quantiser sets.  (a) all 65,536 fp16 bit patterns (its 2,046 NaN patterns included: they must give byte 0).  (b) fp32: for every byte
threshold k = 1..255 the fp32 nearest 2k/255 - 1 (rescale) or k/255 and its +-THRESHOLD_ULPS neighbours - the byte must step from
k - 1 to k somewhere inside each neighbourhood, which is what makes the set a test of the thresholds - plus +-0, +-inf, the smallest
subnormals, +-1, +-2, 1 - 2^-24, 1 + 2^-23 and the largest value below -1.  (c) NaNs, quiet and signalling patterns of both signs,
placed at known cells.

SSIM bounds.  The box moments are exact integers on both sides; the kernel's map value is ~16 fp32 roundings (the count the docstring
of tests/test_gpu_metrics.py derives) of a ratio whose numerator never exceeds its denominator:
    per window    |map - map64|          <=  16 * 2^-24 * max(|map64|, 2^-10)
    per sum       |ssim_sum - sum map64| <=  16 * 2^-24 * npos            (the sums themselves are fp64)
`kernel_double` is the plain-fp32 restatement of the kernel (numpy float32 from the exact integer moments, one rounding per
operation, no contraction); the CPU test feeds it to the very assertions the GPU tests use."""
import numpy as np
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from tests import metrics_ref

WIN = 7
U24 = 2.0 ** -24
ROUNDINGS = 16.0
MAP_FLOOR = 2.0 ** -10
THRESHOLD_ULPS = 8
CLIP = (3, 1, 224, 224)                       # the clip hv_i3d_preprocess passes through pixel by pixel
CLIP_CELLS = 3 * 224 * 224

# ---- quantiser input sets -------------------------------------------------------------------------------------------------------------
NAN_BITS16 = (0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7DFF, 0xFFFF)                  # quiet, signalling patterns, both signs
NAN_BITS32 = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFFFFFFF)


def fp16_all():
    """every fp16 bit pattern, in bit order"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)


def threshold_values(rescale):
    """float32 [255]: the fp32 nearest the input at which the byte steps to k, k = 1..255"""
    k = np.arange(1, 256, dtype=np.float64)
    return (2.0 * k / 255.0 - 1.0 if rescale else k / 255.0).astype(np.float32)


def threshold_neighbourhoods(rescale, ulps=THRESHOLD_ULPS):
    """float32 [255, 4 ulps + 1], ascending along axis 1: each threshold with its +-ulps fp32 neighbours and, under rescale, +-ulps
    steps of the spacing of x + 1 as well.  Near x = 0 (thresholds 124..127) an ulp of x is up to 2^-8 of an ulp of x + 1, the sum the
    byte is formed from: there +-8 ulp of x all round to one sum, the byte stays flat, and the step shows only at the coarser spacing.
    Without rescale the coarse half repeats the fine one."""
    mid = threshold_values(rescale)
    cols = [mid]
    lo = hi = mid
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        cols = [lo] + cols + [hi]
    step = np.spacing(mid + np.float32(1.0)).astype(np.float64) if rescale else np.spacing(mid).astype(np.float64)
    cols += [(mid.astype(np.float64) + j * step).astype(np.float32) for j in range(-ulps, ulps + 1) if j]
    return np.sort(np.stack(cols, axis=1).astype(np.float32), axis=1)


def fp32_specials():
    one = np.float32(1.0)
    sub = np.array([1, 0x80000001], dtype=np.uint32).view(np.float32)
    return np.array([0.0, -0.0, np.inf, -np.inf, sub[0], sub[1], 1.0, -1.0, 2.0, -2.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23,
                     np.nextafter(-one, np.float32(-np.inf))], dtype=np.float32)


def fp32_set(rescale):
    return np.concatenate([threshold_neighbourhoods(rescale).reshape(-1), fp32_specials()])


def nans(dtype):
    if np.dtype(dtype) == np.float16:
        return np.array(NAN_BITS16, dtype=np.uint16).view(np.float16)
    return np.array(NAN_BITS32, dtype=np.uint32).view(np.float32)


def value_set(dtype, rescale):
    """set (a) for fp16, set (b) for fp32"""
    return fp16_all() if np.dtype(dtype) == np.float16 else fp32_set(rescale)


def expected_bytes(x, rescale):
    """uint8 array of x's shape: metrics_ref.quantise, and 0 where x is NaN (the kernels' rule; numpy's cast of NaN is platform-defined
    and is never consulted)"""
    x32 = np.asarray(x).astype(np.float32)
    nan = np.isnan(x32)
    q = metrics_ref.quantise(np.where(nan, np.float32(0.0), x32), rescale)
    q[nan] = 0
    return q


def clip_cells(values, nan_values):
    """-> (flat array of CLIP_CELLS cells: `values` repeated, with the NaNs at known cells, the first and the last among them; the cells
    that hold a NaN of set (c))"""
    flat = np.resize(values, CLIP_CELLS).copy()
    cells = np.array([0, CLIP_CELLS - 1] + [(7919 * (i + 1)) % CLIP_CELLS for i in range(4 * len(nan_values) - 2)], dtype=np.int64)
    assert len(np.unique(cells)) == len(cells)
    flat[cells] = np.resize(nan_values, len(cells))
    return flat, cells


def frames_7x7(values):
    """a flat set as a C = 1 video [1, ceil(n / 49), 7, 7], the tail padded by repeats"""
    T = -(-len(values) // 49)
    return np.resize(values, T * 49).reshape(1, T, 7, 7)


def luma(q, weights):
    """uint8 [3, ...] -> the integer gray value (wr R + wg G + wb B + round) >> shift, int64"""
    wr, wg, wb, rnd, shift = weights
    q = q.astype(np.int64)
    return (wr * q[0] + wg * q[1] + wb * q[2] + rnd) >> shift


# ---- exact integers and fp64 sums of a video pair -------------------------------------------------------------------------------------
def integers(qa, qb):
    """uint8 [C, T, H, W] -> (sse [T] as python integers, minmax [T][4] = min a, max a, min b, max b)"""
    d = qa.astype(np.int64) - qb.astype(np.int64)
    sse = [int(v) for v in (d * d).sum(axis=(0, 2, 3))]
    mm = [[int(qa[:, t].min()), int(qa[:, t].max()), int(qb[:, t].min()), int(qb[:, t].max())] for t in range(qa.shape[1])]
    return sse, mm


class Reference:
    """bytes, exact integers, fp64 SSIM map sums [T, C] and the smallest |map| of a pair of float videos [C, T, H, W]; `R` overrides
    the data range of every frame"""

    def __init__(self, a, b, rescale=True, R=None, ssim=True):
        self.qa, self.qb = expected_bytes(a, rescale), expected_bytes(b, rescale)
        self.sse, self.minmax = integers(self.qa, self.qb)
        C, T, H, W = self.qa.shape
        self.npos = (H - WIN + 1) * (W - WIN + 1)
        if not ssim:
            return
        self.sums = np.zeros((T, C), dtype=np.float64)
        self.min_abs_map = np.inf
        for t in range(T):
            f1, f2 = self.qa[:, t].transpose(1, 2, 0), self.qb[:, t].transpose(1, 2, 0)
            r = (int(f1.max()) - int(f1.min())) if R is None else R
            if r > 0:                                       # the kernel's rule: a constant first frame sums to 0
                maps = metrics_ref.ssim_maps(f1, f2, r)
                self.sums[t] = [m.sum() for m in maps]
                self.min_abs_map = min(self.min_abs_map, float(np.abs(maps).min()))


def ssim_maps_f32(img1, img2, R=None):
    """uint8 [H, W, C] frames -> float32 [C, H-6, W-6]: the kernel's map expression restated in plain fp32, every operation rounded on
    its own, from the exact integer moments; data range of img1's frame over all channels unless given"""
    f = np.float32
    R = (int(img1.max()) - int(img1.min())) if R is None else R
    Rf = f(R)
    C1, C2 = (f(0.01) * Rf) * (f(0.01) * Rf), (f(0.03) * Rf) * (f(0.03) * Rf)
    inv_n2, inv_cov = f(1.0) / f(2401.0), f(1.0) / f(2352.0)
    H, W, C = img1.shape
    out = np.zeros((C, H - WIN + 1, W - WIN + 1), dtype=np.float32)
    for c in range(C):
        sx, sy, sxx, syy, sxy = metrics_ref.box_moments(img1[..., c], img2[..., c])
        pxy = sx * sy
        vx, vy, vxy = 49 * sxx - sx * sx, 49 * syy - sy * sy, 49 * sxy - pxy
        a1 = f(2.0) * pxy.astype(f) * inv_n2 + C1
        b1 = (sx * sx + sy * sy).astype(f) * inv_n2 + C1
        a2 = f(2.0) * vxy.astype(f) * inv_cov + C2
        b2 = (vx + vy).astype(f) * inv_cov + C2
        out[c] = (a1 * a2) / (b1 * b2)
        assert out[c].dtype == np.float32
    return out


def kernel_double(a, b, rescale=True, R=None):
    """what hv_video_metrics returns for float videos [C, T, H, W], restated on the host: sse int64 [T], minmax int32 [T, 4], ssim_sum
    float64 [T, C] (fp32 map values summed in fp64 over the (H-6) x (W-6) window positions; 0 for a constant first frame)"""
    qa, qb = expected_bytes(a, rescale), expected_bytes(b, rescale)
    C, T, H, W = qa.shape
    sse, mm = integers(qa, qb)
    sums = np.zeros((T, C), dtype=np.float64)
    for t in range(T):
        r = (mm[t][1] - mm[t][0]) if R is None else R
        if r > 0:
            maps = ssim_maps_f32(qa[:, t].transpose(1, 2, 0), qb[:, t].transpose(1, 2, 0), r)
            sums[t] = maps.astype(np.float64).sum(axis=(1, 2))
    return {"sse": np.array(sse, dtype=np.int64), "minmax": np.array(mm, dtype=np.int32), "ssim_sum": sums}


# ---- the assertions, shared by the GPU tests and the CPU preconditions ----------------------------------------------------------------
def check_integers(got, ref, tag):
    assert [int(v) for v in got["sse"]] == ref.sse, (tag, "sse")
    assert [[int(v) for v in row] for row in got["minmax"]] == ref.minmax, (tag, "minmax")


def check_census(ssim_sum, H, W, tag):
    """rec is ref: every map value is exactly 1.0f, so the fp64 sum is the window-position count, an exact integer"""
    npos = (H - WIN + 1) * (W - WIN + 1)
    s = np.asarray(ssim_sum, dtype=np.float64)
    assert (s == float(npos)).all(), (tag, npos, s.tolist())


def sum_ratio(ssim_sum, ref):
    """largest |ssim_sum - fp64 sum| over the bound 16 * 2^-24 * npos"""
    d = np.abs(np.asarray(ssim_sum, dtype=np.float64) - ref.sums)
    return float(np.where(np.isfinite(d), d, np.inf).max()) / (ROUNDINGS * U24 * ref.npos)


def window_ratio(ssim_sum, ref):
    """frames of one window position: largest |value - map64| over 16 * 2^-24 * max(|map64|, 2^-10)"""
    assert ref.npos == 1
    d = np.abs(np.asarray(ssim_sum, dtype=np.float64) - ref.sums)
    return float((np.where(np.isfinite(d), d, np.inf) / (ROUNDINGS * U24 * np.maximum(np.abs(ref.sums), MAP_FLOOR))).max())


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def mid_video(shape, key):
    """fp16-representable float32 [C, T, H, W] whose bytes stay inside [50, 200], different content in every frame"""
    return (syn.hashed_uniform(shape, key, 0) * 0.5 - 0.02).half().float().numpy()


def noisy_pair(shape, key):
    """(ref, rec = ref + small noise), bytes inside [50, 200]: every window's SSIM is far from 0"""
    a = mid_video(shape, key + ".a")
    b = (torch.from_numpy(a) + 0.03 * syn.hashed_uniform(shape, key + ".n", 0)).half().float().numpy()
    return a, b


def from_bytes(q):
    """the fp16-representable float32 input at the middle of byte q's interval (rescale on)"""
    x = torch.from_numpy((q.astype(np.float64) + 0.5) / 255.0 * 2.0 - 1.0).half().float().numpy()
    assert np.array_equal(metrics_ref.quantise(x), q.astype(np.uint8))
    return x


def _rand_bytes(shape, key, lo=0, hi=255):
    u = (syn.hashed_uniform(shape, key, 0).double().numpy() + 1.0) / 2.0
    return np.clip(lo + np.floor(u * (hi - lo + 1)), lo, hi).astype(np.int64)


WINDOW_CLASSES = ("random", "noisy", "r1_random", "r1_r1", "checker", "dark", "bright_dark")
WINDOW_T = 512


def _r1(shape, key):
    """every frame holds exactly two byte values, k and k + 1"""
    base = _rand_bytes((1, shape[1], 1, 1), key + ".base", 0, 254)
    bit = _rand_bytes(shape, key + ".bit", 0, 1)
    bit[:, :, 0, 0], bit[:, :, 0, 1] = 0, 1
    return base + bit


def window_class(name, T=WINDOW_T):
    """(a, b) float32 [3, T, 7, 7]: T frames of a single window position each"""
    shape = (3, T, 7, 7)
    key = "metrics.window." + name
    if name == "random":
        qa, qb = _rand_bytes(shape, key + ".a"), _rand_bytes(shape, key + ".b")
    elif name == "noisy":
        qa = _rand_bytes(shape, key + ".a", 50, 200)
        qb = qa + _rand_bytes(shape, key + ".n", -4, 4)
    elif name == "r1_random":
        qa, qb = _r1(shape, key + ".a"), _rand_bytes(shape, key + ".b")
    elif name == "r1_r1":
        qa, qb = _r1(shape, key + ".a"), _r1(shape, key + ".b")
    elif name == "checker":                    # 0 / 255 checkerboards of both phases: the first half against the inverse, then random
        c, t, h, w = np.meshgrid(np.arange(3), np.arange(T), np.arange(7), np.arange(7), indexing="ij")
        qa = 255 * ((c + t + h + w) % 2)
        qb = np.where(t < T // 2, 255 - qa, _rand_bytes(shape, key + ".b"))
    elif name == "dark":
        qa, qb = _rand_bytes(shape, key + ".a", 0, 2), _rand_bytes(shape, key + ".b", 0, 2)
    elif name == "bright_dark":
        qa, qb = _rand_bytes(shape, key + ".a", 200, 255), _rand_bytes(shape, key + ".b", 0, 2)
    else:
        raise KeyError(name)
    return from_bytes(qa), from_bytes(qb)


# ---- case tables ------------------------------------------------------------------------------------------------------------------------------
# pass 2: (C, H, W).  Window positions H-6, W-6 at 1, 31 | 32 | 33, 63 | 64 | 65 and their doubles; several tile rows and columns
TILE_SHAPES = [(3, 7, 7), (3, 7, 70), (3, 38, 7), (3, 37, 69), (3, 38, 70), (3, 39, 71), (3, 39, 135), (3, 71, 134), (1, 70, 199),
               (3, 7, 4103), (1, 1024, 1024)]
# pass 1 chunk count ceil(C H W / 16384) capped at 64: 1 | 2, 64 exactly, the cap with extra trips, the cap with C = 3
CHUNK_SHAPES = [(1, 128, 128), (1, 129, 128), (1, 1024, 1024), (1, 1040, 1024), (3, 600, 600)]
CHUNK_ELEMS, MAX_CHUNKS = 16384, 64


def chunks(C, H, W):
    return min(MAX_CHUNKS, max(1, -(-(C * H * W) // CHUNK_ELEMS)))


def tiles(H, W):
    return -(-(H - 6) // 32), -(-(W - 6) // 64)


def path_cases(vec):
    """pass 1's vector-path predicate, one failing condition at a time: [(tag, side, W, offset, sh, st, sc)] for C = 3, T = 2, H = 8 -
    element strides of a view into one flat buffer, `side` the operand ("a" or "b") that gets this layout while the other keeps the
    baseline's.  vec = 8 (fp16) or 4 (fp32); offset, in elements from a 16-byte-aligned base, is one vector for the baseline"""
    W, H, T = 2 * vec, 8, 2
    sh = W + vec
    st = H * sh + vec
    sc = T * st + vec
    base = ("vector", "a", W, vec, sh, st, sc)
    out = [base]
    for side in ("a", "b"):
        w1 = W + vec // 2
        out += [("W", side, w1, vec, sh, st, sc),                                   # both operands share W: the side is nominal
                ("pointer", side, W, vec + vec // 2, sh, st, sc),
                ("sh", side, W, vec, sh + vec // 2, H * (sh + vec // 2) + (-(H * (sh + vec // 2))) % vec + vec, None),
                ("st", side, W, vec, sh, st + vec // 2, 2 * (st + vec // 2) + (-(2 * (st + vec // 2))) % vec + vec),
                ("sc", side, W, vec, sh, st, sc + vec // 2)]
    fixed = []
    for tag, side, w, off, h, t, c in out:
        c = T * t + (-(T * t)) % vec + vec if c is None else c
        fixed.append((tag, side, w, off, h, t, c))
    return fixed


def vector_path(vec, W, off, sh, st, sc):
    """the launch's predicate for one operand whose buffer base is 16-byte aligned"""
    return W % vec == 0 and off % vec == 0 and sh % vec == 0 and st % vec == 0 and sc % vec == 0
