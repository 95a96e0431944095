"""MXFP6 linears (opt-in; include/hv_gemm_mx6.h): wrappers over torch.ops.hv.quant_rows_mxfp6 / ln_modulate_mxfp6 / gemm_mxfp6.
They are public HERE (hunyuanvideo_efficiency_amd.gemm_mx6), not re-exported through ops: every launching wrapper in the ops namespace
carries a CPU double for the CPU test tier, and this opt-in path has none (tests/mxfp6_ref.py restates its contract for the GPU tests).
Codes are torch.uint8 [rows, 3 K / 4] (32 dense 6-bit e2m3 codes per 24 bytes, element j at bits [6 j, 6 j + 6)), scales torch.uint8 [rows, K / 32] (E8M0)."""
from __future__ import annotations

import torch

from . import _abi, _lib
from .ops import ACT_GELU_TANH, ACT_NONE, ACT_SILU, BF16, _chk, _chk_mod_vectors, _gemm_epilogue, _rows  # noqa: F401  (the ACT_* are public here)

MX6 = _abi.GEMM_MX6_MACROS
U8 = torch.uint8
BLOCK = MX6["HV_MX6_BLOCK"]


def _outputs(m: int, k: int, device, codes, scales):
    if k % BLOCK:
        raise ValueError(f"MXFP6 rows hold whole blocks of {BLOCK}: got K = {k}")
    if codes is None:
        codes = torch.empty(m, k // 4 * 3, dtype=U8, device=device)
    if scales is None:
        scales = torch.empty(m, k // BLOCK, dtype=U8, device=device)
    _chk(codes, U8, "codes"), _chk(scales, U8, "scales")
    mc, kc, ldq = _rows(codes, "codes")
    ms, ks, lds = _rows(scales, "scales")
    assert (mc, kc) == (m, k // 4 * 3) and (ms, ks) == (m, k // BLOCK), (codes.shape, scales.shape, m, k)
    return codes, ldq, scales, lds


def quant_rows_mxfp6(x, codes=None, scales=None):
    """bf16 rows [M, K] -> (codes [M, 3 K / 4], scales [M, K / 32]); also the weight packer (a weight is N rows of K)."""
    _chk(x, BF16, "x")
    m, k, ldx = _rows(x, "x")
    codes, ldq, scales, lds = _outputs(m, k, x.device, codes, scales)
    _lib.call("quant_rows_mxfp6", x, ldx, codes, ldq, scales, lds, m, k)
    return codes, scales


def ln_modulate_mxfp6(x, shift=None, scale=None, codes=None, scales=None, eps: float = 1e-6):
    """bf16(LN(x) * bf16(1 + scale) + shift) quantised by the same rule, without the bf16 rows reaching HBM."""
    _chk(x, BF16, "x")
    m, d, ldx = _rows(x, "x")
    codes, ldq, scales, lds = _outputs(m, d, x.device, codes, scales)
    _chk_mod_vectors(shift, scale, d)
    _lib.call("ln_modulate_mxfp6", x, shift, scale, codes, ldq, scales, lds, m, d, ldx, eps)
    return codes, scales


def gemm_mxfp6(a_codes, a_scales, w_codes, w_scales, bias=None, out=None, act: int = ACT_NONE, n_split: int = 0, out1=None,
               act1: int = ACT_NONE, gate=None, res=None):
    """out = dequant(a) @ dequant(w).T + bias with hv_gemm_bf16's epilogues; the block scales are applied by the matrix instruction."""
    for t, nm in ((a_codes, "a_codes"), (a_scales, "a_scales"), (w_codes, "w_codes"), (w_scales, "w_scales")):
        _chk(t, U8, nm)
    m, kb, lda = _rows(a_codes, "a_codes")
    n, kbw, ldw = _rows(w_codes, "w_codes")
    ms, nb, ldas = _rows(a_scales, "a_scales")
    ns, nbw, ldws = _rows(w_scales, "w_scales")
    k = kb // 3 * 4
    assert kb == kbw and kb % 3 == 0 and ms == m and ns == n and nb == nbw == k // BLOCK, (a_codes.shape, a_scales.shape, w_codes.shape, w_scales.shape)
    out, n0, ld0, ld1, ld_res = _gemm_epilogue((m,), a_codes.device, m, n, n_split, out, out1, bias, gate, res)
    _lib.call("gemm_mxfp6", a_codes, lda, a_scales, ldas, w_codes, ldw, w_scales, ldws, bias, m, n, k, out, ld0, act, n0, out1, ld1,
              act1, gate, res, ld_res)
    return out
