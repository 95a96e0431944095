"""numpy int64 restatement of the video tensor -> raw YUV 4:2:0 rules (include/hv_yuv_write.h, hv_clip_to_yuv420), written from their
statement and not from the kernel: the quantiser, BT.601 limited-range fixed-point colour, both chroma modes, the three layouts.
UNPINNED RESTATEMENT, like the header: cv2 cannot be executed here, parity with its bytes is not claimed."""
import numpy as np
import torch

CHROMA = {"topleft": 0, "mean": 1}


def quantise(x: torch.Tensor, rescale: bool) -> np.ndarray:
    """host tensor (fp16 / fp32) -> int64 bytes: float(); (v + 1.0) / 2.0 if rescale; clamp(0, 1); * 255, every step in fp32; truncate;
    NaN -> 0 (utils/file_utils.py:frames_uint8 for every finite value)"""
    v = x.detach().cpu().float().numpy().astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if rescale:
            v = ((v + np.float32(1.0)) / np.float32(2.0)).astype(np.float32)
        nan = np.isnan(v)
        v = np.minimum(np.maximum(np.where(nan, np.float32(0), v), np.float32(0)), np.float32(1))
        q = (v * np.float32(255.0)).astype(np.float32).astype(np.int64)
    q[nan] = 0
    return q


def luma(R, G, B):
    return (269484 * R + 528482 * G + 102760 * B + (16 << 20) + (1 << 19)) >> 20


def chroma_uv(R, G, B, shift=20):
    """shift = 20: one pixel's bytes; 22: the sums of the four pixels of a block"""
    half, mid = 1 << (shift - 1), 128 << shift
    return ((-155188 * R - 305135 * G + 460324 * B + mid + half) >> shift,
            (460324 * R - 385875 * G - 74448 * B + mid + half) >> shift)


def yuv_planes(q: np.ndarray, chroma: str):
    """q int64 [C, T, H, W] of bytes, C = 1 | 3 -> (Y [T,H,W], U [T,H/2,W/2], V [T,H/2,W/2]) int64"""
    R, G, B = (q[0], q[0], q[0]) if q.shape[0] == 1 else (q[0], q[1], q[2])
    Y = luma(R, G, B)
    if chroma == "topleft":
        U, V = chroma_uv(R[:, ::2, ::2], G[:, ::2, ::2], B[:, ::2, ::2])
    else:
        assert chroma == "mean"
        s = lambda p: p[:, ::2, ::2] + p[:, ::2, 1::2] + p[:, 1::2, ::2] + p[:, 1::2, 1::2]
        U, V = chroma_uv(s(R), s(G), s(B), 22)
    return Y, U, V


def pack(Y, U, V, fmt: str) -> np.ndarray:
    """-> uint8 [T, W*H*3/2] in layout fmt"""
    T = Y.shape[0]
    for p, lo, hi in ((Y, 16, 235), (U, 16, 240), (V, 16, 240)):
        assert p.min() >= lo and p.max() <= hi
    y, u, v = Y.reshape(T, -1), U.reshape(T, -1), V.reshape(T, -1)
    if fmt == "I420":
        parts = [y, u, v]
    elif fmt == "YV12":
        parts = [y, v, u]
    else:
        assert fmt == "NV12"
        parts = [y, np.stack([u, v], axis=2).reshape(T, -1)]
    return np.concatenate(parts, axis=1).astype(np.uint8)


def frames(x: torch.Tensor, fmt: str = "I420", rescale: bool = False, chroma: str = "mean") -> np.ndarray:
    """x [C, T, H, W] -> uint8 [T, W*H*3/2]"""
    return pack(*yuv_planes(quantise(x, rescale), chroma), fmt)


def y4m_bytes(x: torch.Tensor, fps_num: int, fps_den: int, rescale: bool = False, chroma: str = "mean") -> bytes:
    """the whole .y4m file of x"""
    C, T, H, W = x.shape
    head = f"YUV4MPEG2 W{W} H{H} F{fps_num}:{fps_den} Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode()
    return head + b"".join(b"FRAME\n" + f.tobytes() for f in frames(x, "I420", rescale, chroma))


def edge_values(shape, dtype, rescale: bool, seed: int) -> torch.Tensor:
    """test input: values around every quantiser step - exact half-codes and code boundaries k / 255 and their neighbours -, values
    outside the range, and NaN, +inf, -inf sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    k = torch.randint(0, 256, (n,), generator=g).float()
    kind = torch.randint(0, 8, (n,), generator=g)
    v = torch.where(kind == 0, (k + 0.5) / 255, torch.where(kind == 1, k / 255, (k + torch.rand(n, generator=g)) / 255))
    v = torch.where(kind == 2, v + 1.5, torch.where(kind == 3, v - 1.5, v))
    if rescale:
        v = v * 2 - 1
    special = torch.randint(0, 97, (n,), generator=g)
    v[special == 0] = float("nan")
    v[special == 1] = float("inf")
    v[special == 2] = float("-inf")
    return v.reshape(shape).to(dtype)
