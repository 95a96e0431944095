"""A torch restatement of include/hv_mx_rot.h, written from the header: the staged fp32 Walsh-Hadamard rotation over groups of R
consecutive k (every stage one rounded fp32 add or subtract per element, then the exact power-of-two factor), composed with the MXFP4
quantiser of tests/mxfp4_ref.py, and the rotation-aware precision object of the model-level test."""
import torch
import torch.nn.functional as F

from tests import mxfp4_ref as MX


def wht(x, rot):
    """x [M, K] (bf16 or bf16-valued fp32), K % rot == 0 -> fp32 [M, K]"""
    y = x.float().cpu()
    m, k = y.shape
    for s in range(rot.bit_length() - 1):
        p = y.reshape(m, k >> (s + 1), 2, 1 << s)              # [.., 0, :] = the elements with bit s clear, [.., 1, :] their partners
        y = torch.stack([p[:, :, 0] + p[:, :, 1], p[:, :, 0] - p[:, :, 1]], dim=2).reshape(m, k)
    return y * 2.0 ** -((rot.bit_length() - 1) // 2)


def quant_rows(x, rot):
    return MX.quant_rows(wht(x, rot))


class Mxfp4RotPrec(MX.Mxfp4Prec):
    """Mxfp4Prec with both operands rotated: a weight registered with `mx` holds dequant(Q(W H)), the activation is Q(bf16(x) H)."""

    def __init__(self, rot):
        super().__init__()
        self.rot = rot

    def linear(self, x, w, b):
        if id(w) not in self._mx:
            return super().linear(x, w, b)
        xr = self.r(x)
        q = MX.dequant(*quant_rows(xr.reshape(-1, xr.shape[-1]), self.rot)).reshape(xr.shape)
        return self.r(F.linear(q, w, None if b is None else self.r(b)))
