"""A torch restatement of include/hv_gemm_mx4.h, written from the header: the MXFP4 quantiser (bf16 rows -> e2m1 codes, two per byte
with the low nibble first, + one E8M0 scale per 32 elements), the exact dequantiser, and the quantisation-aware precision object of the
model-level test.  Everything is integer work on fp32 bit patterns or exact fp64 arithmetic."""
import torch
import torch.nn.functional as F

from oracle import dit_ref as R

VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
# midpoints between neighbouring magnitudes; a tie goes to the even index: up at 0.75, 1.75, 3.5 (>=), down at 0.25, 1.25, 2.5, 5 (>)
MID = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def quant_rows(x):
    """x [M, K] (bf16 or bf16-valued fp32), K % 32 == 0 -> (codes uint8 [M, K / 2], scales uint8 [M, K / 32])"""
    x = x.float().cpu()
    m, k = x.shape
    bits = x.view(torch.int32).reshape(m, k // 32, 32)
    E = ((bits & 0x7FFFFFFF).amax(dim=-1) >> 23)                       # exponent field of the block's largest magnitude
    e = (E - 2).clamp(min=0)
    v = x.double().reshape(m, k // 32, 32).abs() * torch.exp2((127 - e).double())[..., None]      # exact in fp64
    idx = torch.zeros_like(v, dtype=torch.int32)
    for mid, up in MID:
        idx += (v >= mid).int() if up else (v > mid).int()
    code = torch.where(idx > 0, idx | ((bits >> 28) & 8), idx).reshape(m, k)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8), e.to(torch.uint8)


def dequant(codes, scales):
    """-> fp32 [M, K], exact (a 2-bit significand times a power of two)"""
    c = codes.cpu().int()
    code = torch.stack([c & 15, c >> 4], dim=-1).reshape(c.shape[0], -1)
    val = VALUES[(code & 7).long()] * torch.where((code & 8) != 0, -1.0, 1.0)
    return (val * torch.exp2(scales.cpu().double() - 127).repeat_interleave(32, dim=1)).float()


class Mxfp4Prec(R.Prec):
    """bf16-emulated contract + MXFP4 Linears: a weight registered with `mx(codes, scales)` is multiplied as
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
