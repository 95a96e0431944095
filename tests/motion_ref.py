"""numpy restatement (integers only, int64) of the block-matching motion field of csrc/hv_motion.hip (include/hv_motion.h has the
definition).  The gray byte is the one the content statistics use (tests/content_ref.gray_frames: utils.file_utils.frames_uint8, then the
integer luma).

The measure is this project's own and is not FVMD: dense full-search block matching on 8-bit gray frames.  Blocks of B x B pixels tile
frame t + 1 from (0, 0), edge blocks are partial; for a displacement (dy, dx) in [-R, R]^2
    SAD  = sum |g[t + 1][y][x] - g[t][clamp(y + dy)][clamp(x + dx)]|          (replicated edges)
    cost = SAD + lam (|dy| + |dx|)
and the winner is the minimum under the lexicographic order (cost, dy^2 + dx^2, dy, dx).  The candidates are visited in ascending
(dy, dx) and replace the best only when (cost, norm) is strictly smaller, which is that order without any packed key."""
import numpy as np

from tests.content_ref import gray_frames
from tests.spectrum_ref import GRAY_LUMA

DEFINITION = ("full-search block matching on 8-bit gray frames (SAD + lam (|dy| + |dx|), ties to the shorter vector), px/frame; this "
              "project's own measure, not FVMD")


def default_lam(block):
    return block * block // 16


def blocks(H, W, block):
    return -(-H // block), -(-W // block)


def block_motion_of_gray(g, block=16, radius=16, lam=None):
    """g integer [T, H, W] in 0..255 -> (mv int16 [T-1, Hb, Wb, 2], sad uint32 [T-1, Hb, Wb], sad0 uint32 [T-1, Hb, Wb])"""
    g = np.asarray(g).astype(np.int64)
    assert g.ndim == 3 and g.min() >= 0 and g.max() <= 255
    assert block in (8, 16) and 1 <= radius <= 32
    lam = default_lam(block) if lam is None else int(lam)
    assert 0 <= lam <= 255
    T, H, W = g.shape
    Hb, Wb = blocks(H, W, block)
    R = radius
    ys, xs = np.arange(0, H, block), np.arange(0, W, block)
    mv = np.zeros((max(T - 1, 0), Hb, Wb, 2), dtype=np.int16)
    sad = np.zeros((max(T - 1, 0), Hb, Wb), dtype=np.uint32)
    sad0 = np.zeros_like(sad)
    for t in range(T - 1):
        prev, cur = np.pad(g[t], R, mode="edge"), g[t + 1]
        best_cost = np.full((Hb, Wb), np.iinfo(np.int64).max, dtype=np.int64)
        best_norm = np.zeros((Hb, Wb), dtype=np.int64)
        best_sad = np.zeros((Hb, Wb), dtype=np.int64)
        best_dy = np.zeros((Hb, Wb), dtype=np.int64)
        best_dx = np.zeros((Hb, Wb), dtype=np.int64)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                d = np.abs(cur - prev[R + dy:R + dy + H, R + dx:R + dx + W])
                s = np.add.reduceat(np.add.reduceat(d, ys, axis=0), xs, axis=1)
                cost, norm = s + lam * (abs(dy) + abs(dx)), dy * dy + dx * dx
                better = (cost < best_cost) | ((cost == best_cost) & (norm < best_norm))
                best_cost = np.where(better, cost, best_cost)
                best_norm = np.where(better, norm, best_norm)
                best_sad = np.where(better, s, best_sad)
                best_dy = np.where(better, dy, best_dy)
                best_dx = np.where(better, dx, best_dx)
                if dy == 0 and dx == 0:
                    sad0[t] = s
        mv[t, :, :, 0], mv[t, :, :, 1], sad[t] = best_dy, best_dx, best_sad
    return mv, sad, sad0


def block_motion(x, block=16, radius=16, lam=None, rescale=True, luma=GRAY_LUMA):
    """float array [3, T, H, W] -> (mv, sad, sad0)"""
    x = np.asarray(x)
    _, T, H, W = x.shape
    return block_motion_of_gray(gray_frames(x, rescale, luma).reshape(T, H, W), block, radius, lam)


def shifted(P, sy, sx):
    """cur[y][x] = P[clamp(y + sy)][clamp(x + sx)]"""
    P = np.asarray(P)
    H, W = P.shape
    yy = np.clip(np.arange(H) + sy, 0, H - 1)
    xx = np.clip(np.arange(W) + sx, 0, W - 1)
    return P[yy][:, xx]
