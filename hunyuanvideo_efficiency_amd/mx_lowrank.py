"""MXFP4 linears with a low-rank bf16 branch (opt-in; include/hv_mx_lowrank.h): wrappers over torch.ops.hv.quant_rows_mxfp4_lr /
gemm_mxfp4_lr, and the factorisation W = Up . Dn + Res that feeds them.  y = Q4(A) Q4(Res)^T + bf16(A Dn^T) Up^T: the first call
quantises A and produces T = bf16(A Dn^T) in one pass, the second folds T Up^T into the GEMM's accumulators.  Public HERE, not
re-exported through ops, for the reason gemm_mx4 gives (no CPU double; tests/mx_lowrank_ref.py restates the contract for the GPU tests)."""
from __future__ import annotations

import torch

from . import _abi, _lib
from .gemm_mx4 import U8, _outputs
from .ops import ACT_NONE, BF16, _chk, _gemm_epilogue, _rows

CHUNK, MAX_RANK = _abi.MX_LOWRANK_MACROS["HV_MX_LR_CHUNK"], _abi.MX_LOWRANK_MACROS["HV_MX_LR_MAX"]
RANKS = tuple(range(CHUNK, MAX_RANK + 1, CHUNK))


def _chk_rank(r: int):
    if r not in RANKS:
        raise ValueError(f"the rank must be one of {RANKS}, got {r}")


def factorise(w, rank: int):
    """bf16 W [N, K] -> (Up [N, R], Dn [R, K], Res [N, K]), all bf16: the R leading singular directions of W (fp32 SVD, on W's device
    or on the CPU where the ROCm build has no SVD), Up = bf16(U_R S_R), Dn = bf16(V_R^T), Res = bf16(W - Up Dn)."""
    _chk_rank(rank)
    wf = w.float()
    try:
        u, s, vh = torch.linalg.svd(wf, full_matrices=False)
    except RuntimeError:
        u, s, vh = (t.to(w.device) for t in torch.linalg.svd(wf.cpu(), full_matrices=False))
    up, dn = (u[:, :rank] * s[:rank]).to(BF16), vh[:rank].to(BF16)
    return up.contiguous(), dn.contiguous(), (wf - up.float() @ dn.float()).to(BF16)


def quant_rows_mxfp4_lr(x, dn, codes=None, scales=None, t=None):
    """bf16 rows [M, K], Dn [R, K] -> (codes [M, K / 2], scales [M, K / 32], T [M, R] = bf16(x Dn^T)); K % 128 == 0"""
    _chk(x, BF16, "x"), _chk(dn, BF16, "dn")
    m, k, ldx = _rows(x, "x")
    r, kd, ldd = _rows(dn, "dn")
    _chk_rank(r)
    assert kd == k, (x.shape, dn.shape)
    codes, ldq, scales, lds = _outputs(m, k, x.device, codes, scales)
    if t is None:
        t = torch.empty(m, r, dtype=BF16, device=x.device)
    _chk(t, BF16, "t")
    mt, rt, ldt = _rows(t, "t")
    assert (mt, rt) == (m, r), (t.shape, m, r)
    _lib.call("quant_rows_mxfp4_lr", x, ldx, codes, ldq, scales, lds, dn, ldd, t, ldt, m, k, r)
    return codes, scales, t


def gemm_mxfp4_lr(a_codes, a_scales, w_codes, w_scales, t, up, bias=None, out=None, act: int = ACT_NONE, n_split: int = 0, out1=None,
                  act1: int = ACT_NONE, gate=None, res=None):
    """out = dequant(a) @ dequant(w).T + t @ up.T + bias with hv_gemm_bf16's epilogues (gemm_mx4.gemm_mxfp4 + the rank-R term)"""
    for x, nm in ((a_codes, "a_codes"), (a_scales, "a_scales"), (w_codes, "w_codes"), (w_scales, "w_scales")):
        _chk(x, U8, nm)
    _chk(t, BF16, "t"), _chk(up, BF16, "up")
    m, kb, lda = _rows(a_codes, "a_codes")
    n, kbw, ldw = _rows(w_codes, "w_codes")
    ms, nb, ldas = _rows(a_scales, "a_scales")
    ns, nbw, ldws = _rows(w_scales, "w_scales")
    mt, r, ldt = _rows(t, "t")
    nu, ru, ldu = _rows(up, "up")
    _chk_rank(r)
    k = 2 * kb
    assert kb == kbw and ms == m and ns == n and nb == nbw == k // 32 and mt == m and nu == n and ru == r, \
        (a_codes.shape, a_scales.shape, w_codes.shape, w_scales.shape, t.shape, up.shape)
    out, n0, ld0, ld1, ld_res = _gemm_epilogue((m,), a_codes.device, m, n, n_split, out, out1, bias, gate, res)
    _lib.call("gemm_mxfp4_lr", a_codes, lda, a_scales, ldas, w_codes, ldw, w_scales, ldws, bias, m, n, k, out, ld0, act, n0, out1, ld1,
              act1, gate, res, ld_res, t, ldt, up, ldu, r)
    return out
