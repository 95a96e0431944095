"""A torch restatement of include/hv_mx_lowrank.h, written from the header: the factorisation W = Up Dn + Res and the precision object of
the model-level test, whose packed Linears add the bf16 rank-R branch to tests/mxfp4_ref.py's MXFP4 product."""
import torch
import torch.nn.functional as F

from tests import mxfp4_ref as MX

BF = torch.bfloat16


def factorise(w, rank):
    """bf16 W [N, K] -> (Up, Dn, Res) bf16: Up = bf16(U_R S_R), Dn = bf16(V_R^T), Res = bf16(W - Up Dn), fp32 SVD on the CPU"""
    wf = w.float().cpu()
    u, s, vh = torch.linalg.svd(wf, full_matrices=False)
    up, dn = (u[:, :rank] * s[:rank]).to(BF).contiguous(), vh[:rank].to(BF).contiguous()
    return up, dn, (wf - up.float() @ dn.float()).to(BF)


class Mxfp4LowrankPrec(MX.Mxfp4Prec):
    """Mxfp4Prec whose packed Linears carry a branch: `mx_lr(codes, scales, up, dn)` registers dequant(Q(Res)) with its Up and Dn, and
    y = bf16(dequant(Q(bf16(x))) . w^T + bf16(bf16(x) . Dn^T) . Up^T + b)"""

    def mx_lr(self, codes, scales, up, dn):
        w = self.mx(codes, scales)
        self._mx[id(w)] = (up.float().cpu(), dn.float().cpu())
        return w

    def linear(self, x, w, b):
        if id(w) not in self._mx:
            return super().linear(x, w, b)
        r, (up, dn) = self.r, self._mx[id(w)]
        xr = r(x)
        q = MX.dequant(*MX.quant_rows(xr.reshape(-1, xr.shape[-1]))).reshape(xr.shape)
        return r(F.linear(q, w, None if b is None else r(b)) + F.linear(r(F.linear(xr, dn)), up))
