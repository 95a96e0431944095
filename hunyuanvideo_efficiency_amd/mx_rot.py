"""MXFP4 linears, rotated operands (opt-in; include/hv_mx_rot.h): wrappers over torch.ops.hv.quant_rows_mxfp4_rot /
ln_modulate_mxfp4_rot, the quantisers of gemm_mx4 behind a block-diagonal Hadamard rotation over groups of `rot` consecutive k.  Both
operands of a gemm_mx4.gemm_mxfp4 call go through them with the same rot: (A H)(W H)^T = A W^T.  Public HERE, not re-exported through
ops, for the reason gemm_mx4 gives (no CPU double; tests/mx_rot_ref.py restates the contract for the GPU tests)."""
from __future__ import annotations

from . import _lib
from .gemm_mx4 import _outputs
from .ops import BF16, _chk, _chk_mod_vectors, _rows

ROTS = (16, 64, 256)


def _chk_rot(rot: int, k: int):
    if rot not in ROTS or k % rot:
        raise ValueError(f"rot must be one of {ROTS} and divide K: got rot = {rot}, K = {k}")


def quant_rows_mxfp4_rot(x, rot: int = 64, codes=None, scales=None):
    """bf16 rows [M, K] -> (codes [M, K / 2], scales [M, K / 32]) of the rotated rows; also the weight packer."""
    _chk(x, BF16, "x")
    m, k, ldx = _rows(x, "x")
    _chk_rot(rot, k)
    codes, ldq, scales, lds = _outputs(m, k, x.device, codes, scales)
    _lib.call("quant_rows_mxfp4_rot", x, ldx, codes, ldq, scales, lds, m, k, rot)
    return codes, scales


def ln_modulate_mxfp4_rot(x, shift=None, scale=None, rot: int = 64, codes=None, scales=None, eps: float = 1e-6):
    """bf16(LN(x) * bf16(1 + scale) + shift), rotated and quantised, without the bf16 rows reaching HBM."""
    _chk(x, BF16, "x")
    m, d, ldx = _rows(x, "x")
    _chk_rot(rot, d)
    codes, ldq, scales, lds = _outputs(m, d, x.device, codes, scales)
    _chk_mod_vectors(shift, scale, d)
    _lib.call("ln_modulate_mxfp4_rot", x, shift, scale, codes, ldq, scales, lds, m, d, ldx, eps, rot)
    return codes, scales
