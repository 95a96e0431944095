"""A torch restatement of include/hv_gemm_mx6.h, written from the header: the MXFP6 quantiser (bf16 rows -> dense 6-bit e2m3 codes,
element j of a block at bits [6 j, 6 j + 6) of its 24 bytes, + one E8M0 scale per 32 elements), the exact dequantiser, and the
quantisation-aware precision object of the model-level test.  Everything is integer work on fp32 bit patterns or exact fp64 arithmetic."""
import torch
import torch.nn.functional as F

from oracle import dit_ref as R

# magnitude index i: i / 8 below 8, (1 + (i & 7) / 8) * 2^((i >> 3) - 1) from 8 on
VALUES = torch.tensor([i / 8 if i < 8 else (1 + (i & 7) / 8) * 2.0 ** ((i >> 3) - 1) for i in range(32)], dtype=torch.float64)
# midpoints between neighbouring magnitudes; a tie goes to the even index: up (>=) into an even index, down (>) out of one
MID = [((float(VALUES[i]) + float(VALUES[i + 1])) / 2, i % 2 == 1) for i in range(31)]


def pack(code):
    """6-bit codes int [M, K] -> uint8 [M, 3 K / 4]: four codes c0 .. c3 are the 24-bit little-endian integer c0 | c1 << 6 | c2 << 12 | c3 << 18"""
    c = code.long().reshape(code.shape[0], -1, 4)
    w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    return torch.stack([w & 255, (w >> 8) & 255, w >> 16], dim=-1).reshape(code.shape[0], -1).to(torch.uint8)


def unpack(codes):
    b = codes.cpu().long().reshape(codes.shape[0], -1, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([(w >> s) & 63 for s in (0, 6, 12, 18)], dim=-1).reshape(codes.shape[0], -1)


def quant_rows(x):
    """x [M, K] (bf16 or bf16-valued fp32), K % 32 == 0 -> (codes uint8 [M, 3 K / 4], scales uint8 [M, K / 32])"""
    x = x.float().cpu()
    m, k = x.shape
    bits = x.view(torch.int32).reshape(m, k // 32, 32)
    E = ((bits & 0x7FFFFFFF).amax(dim=-1) >> 23)                       # exponent field of the block's largest magnitude
    e = (E - 2).clamp(min=0)
    v = x.double().reshape(m, k // 32, 32).abs() * torch.exp2((127 - e).double())[..., None]      # exact in fp64
    idx = torch.zeros_like(v, dtype=torch.int32)
    for mid, up in MID:
        idx += (v >= mid).int() if up else (v > mid).int()
    code = torch.where(idx > 0, idx | ((bits >> 26) & 32), idx).reshape(m, k)
    return pack(code), e.to(torch.uint8)


def dequant(codes, scales):
    """-> fp32 [M, K], exact (a 4-bit significand times a power of two)"""
    code = unpack(codes)
    val = VALUES[code & 31] * torch.where((code & 32) != 0, -1.0, 1.0)
    return (val * torch.exp2(scales.cpu().double() - 127).repeat_interleave(32, dim=1)).float()


class Mxfp6Prec(R.Prec):
    """bf16-emulated contract + MXFP6 Linears: a weight registered with `mx(codes, scales)` is multiplied as
    y = bf16(dequant(Q(bf16(x))) . dequant(w)^T + b); every other Linear follows Prec(True)."""

    def __init__(self):
        super().__init__(True)
        self._mx = {}

    def mx(self, codes, scales):
        w = dequant(codes, scales)
        self._mx[id(w)] = True
        return w

    def linear(self, x, w, b):
        if id(w) not in self._mx:
            return super().linear(x, w, b)
        xr = self.r(x)
        q = dequant(*quant_rows(xr.reshape(-1, xr.shape[-1]))).reshape(xr.shape)
        return self.r(F.linear(q, w, None if b is None else self.r(b)))
