"""numpy int64 restatement of the raw YUV 4:2:0 -> clip rules (include/hv_kernels.h, hv_yuv420_to_clip), written from their statement and
not from the kernel: layouts, BT.601 limited-range fixed-point colour, the table-driven 2-tap bilinear resize and the value table."""
import numpy as np
import torch

COEF = 2048


def planes(frames: np.ndarray, W: int, H: int, fmt: str):
    """frames uint8 [T, W*H*3/2] -> (Y [T,H,W], U [T,H/2,W/2], V [T,H/2,W/2]) as int64"""
    T = frames.shape[0]
    n, q = W * H, W * H // 4
    Y = frames[:, :n].reshape(T, H, W).astype(np.int64)
    if fmt == "NV12":
        uv = frames[:, n:].reshape(T, H // 2, W // 2, 2).astype(np.int64)
        return Y, uv[..., 0], uv[..., 1]
    a = frames[:, n:n + q].reshape(T, H // 2, W // 2).astype(np.int64)
    b = frames[:, n + q:].reshape(T, H // 2, W // 2).astype(np.int64)
    return (Y, a, b) if fmt == "I420" else (Y, b, a)


def colour(Y, U, V):
    """int64 arrays of equal shape -> (R, G, B) bytes"""
    yy = np.maximum(0, Y - 16) * 1220542
    u, v = U - 128, V - 128
    r = np.clip((yy + 1673527 * v + (1 << 19)) >> 20, 0, 255)
    g = np.clip((yy - 852492 * v - 409993 * u + (1 << 19)) >> 20, 0, 255)
    b = np.clip((yy + 2116026 * u + (1 << 19)) >> 20, 0, 255)
    return r, g, b


def rgb_frames(frames: np.ndarray, W: int, H: int, fmt: str) -> np.ndarray:
    """-> int64 [3, T, H, W], channel order R, G, B; pixel (y, x) uses chroma sample (y >> 1, x >> 1)"""
    Y, U, V = planes(frames, W, H, fmt)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)
    return np.stack(colour(Y, up(U), up(V)))


def axis_table(src: int, dst: int):
    """-> (i0, i1, c0, c1) int64 [dst]"""
    i0, i1, c0, c1 = (np.zeros(dst, dtype=np.int64) for _ in range(4))
    for d in range(dst):
        f = np.float32((d + 0.5) * (src / dst) - 0.5)
        s = int(np.floor(f))
        a = np.float32(f - np.float32(s))
        if s < 0 or s >= src - 1:
            s = min(max(s, 0), src - 1)
            a = np.float32(0.0)
        w = int(np.rint(np.float32(a * np.float32(COEF))))
        i0[d], i1[d], c0[d], c1[d] = s, min(s + 1, src - 1), COEF - w, w
    return i0, i1, c0, c1


def resize(img: np.ndarray, OH: int, OW: int) -> np.ndarray:
    """img int64 [..., H, W] of bytes -> [..., OH, OW]; equal sizes: the image itself (no tables, no taps)"""
    H, W = img.shape[-2:]
    if (OH, OW) == (H, W):
        return img
    y0, y1, cy0, cy1 = axis_table(H, OH)
    x0, x1, cx0, cx1 = axis_table(W, OW)
    h0 = cx0 * img[..., y0, :][..., x0] + cx1 * img[..., y0, :][..., x1]
    h1 = cx0 * img[..., y1, :][..., x0] + cx1 * img[..., y1, :][..., x1]
    return (cy0[:, None] * h0 + cy1[:, None] * h1 + (1 << 21)) >> 22


def value_table(dtype) -> torch.Tensor:
    rows = [(torch.tensor(q, dtype=torch.uint8).float() / 255) * 2 - 1 for q in range(256)]
    return torch.stack(rows).to(dtype)


def clip(frames: np.ndarray, W: int, H: int, fmt: str, dtype, size=None) -> torch.Tensor:
    """frames uint8 [T, W*H*3/2]; size = (OW, OH) or None -> [3, T, OH, OW] of `dtype` on the host"""
    q = rgb_frames(frames, W, H, fmt)
    if size is not None:
        q = resize(q, size[1], size[0])
    return value_table(dtype)[torch.from_numpy(np.ascontiguousarray(q))]
