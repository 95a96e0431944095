"""Tensor-level wrappers of the FP8 attention forward (include/hv_attn_fp8.h, csrc/hv_attn_fp8.hip; opt-in), public as ops.attn_fwd_fp8,
ops.attn_fp8_quantise, ops.attn_fp8_workspace_bytes and ops.attn_fp8_layout.  GPU tensors only, like every wrapper of ops.py."""
from __future__ import annotations

from typing import Optional

import torch

from . import _abi, _lib

ATTN_FP8 = _abi.ATTN_FP8_MACROS     # HV_ATTN_FP8_BM / _RING / _KVT / _STAT_KEYS / _ALIGN of include/hv_attn_fp8.h


def attn_fp8_workspace_bytes(n_q: int, n_kv: int, n_heads: int) -> int:
    return int(_lib.host("attn_fp8_workspace_bytes", n_q, n_kv, n_heads))


def attn_fp8_layout(n_q: int, n_kv: int, n_heads: int) -> dict:
    """Byte offsets of the workspace areas of include/hv_attn_fp8.h (and "total", "nt", "nb"), restated from its layout paragraph."""
    al, nt, nb = ATTN_FP8["HV_ATTN_FP8_ALIGN"], -(-n_kv // ATTN_FP8["HV_ATTN_FP8_KVT"]), -(-n_kv // ATTN_FP8["HV_ATTN_FP8_STAT_KEYS"])
    sizes = (("kmean", n_heads * 512), ("sv", n_heads * 512), ("sk", n_heads * nt * 4), ("sq", n_q * n_heads * 4),
             ("part", n_heads * nb * 1024), ("q8", n_q * n_heads * 128), ("k8", n_heads * nt * 8192), ("v8", n_heads * nt * 8192))
    out, at = {"nt": nt, "nb": nb}, 0
    for name, size in sizes:
        out[name] = at
        at = -(-(at + size) // al) * al
    out["total"] = at
    return out


def _attn_fp8_args(q, k, v, n_heads, workspace):
    from .ops import BF16, _chk
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        _chk(t, BF16, nm)
        assert t.dim() == 2
    n_q, n_kv = q.shape[0], k.shape[0]
    assert v.shape[0] == n_kv
    need = attn_fp8_workspace_bytes(n_q, n_kv, n_heads)
    if need == 0 and n_q > 0:
        raise ValueError(f"attn_fwd_fp8: extents n_q {n_q}, n_kv {n_kv}, n_heads {n_heads} are outside include/hv_attn_fp8.h")
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=q.device)
    _chk(workspace, torch.uint8, "workspace")
    if workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"attn_fwd_fp8: workspace must be a contiguous uint8 vector of at least {need} bytes, got {tuple(workspace.shape)}")
    return n_q, n_kv, workspace


def attn_fp8_quantise(q, k, v, n_heads: int, scale: Optional[float] = None, workspace=None):
    """hv_attn_fp8_quantise: bf16 q [n_q, >= H*128], k, v [n_kv, ..] (2-D views, head h at column h*128) -> the workspace of
    include/hv_attn_fp8.h (allocated when None, reused when given); returns it."""
    n_q, n_kv, workspace = _attn_fp8_args(q, k, v, n_heads, workspace)
    _lib.call("attn_fp8_quantise", q, k, v, q.stride(0), k.stride(0), v.stride(0), n_q, n_kv, n_heads, 128,
              128 ** -0.5 if scale is None else scale, workspace, workspace.numel())
    return workspace


def attn_fwd_fp8(q, k, v, out, n_heads: int, scale: Optional[float] = None, workspace=None):
    """attn_fwd with Q, K, V and P in e4m3 on the scaled f8f6f4 MFMA (opt-in; include/hv_attn_fp8.h): quantise into the workspace,
    then the attention kernel.  Same arguments and checks as attn_fwd."""
    from .ops import BF16, _chk
    _chk(out, BF16, "out")
    assert out.dim() == 2 and out.shape[0] == q.shape[0]
    workspace = attn_fp8_quantise(q, k, v, n_heads, scale, workspace)
    _lib.call("attn_fwd_fp8", workspace, workspace.numel(), out, out.stride(0), q.shape[0], k.shape[0], n_heads, 128)
    return out
