"""MXFP6 linears (opt-in; include/hv_gemm_mx6.h): pack the block GEMM weights as dense 6-bit e2m3 codes + E8M0 block scales and run
them, with activations quantised the same way, on v_mfma_scale_f32_16x16x128_f8f6f4.  Not the reference's arithmetic: round-to-nearest
e2m3 carries about 2.8 % relative noise per element (e4m3's 3 mantissa bits; e2m1 carries 11 %); no run on real weights has measured
video fidelity under it."""
from __future__ import annotations

import torch

from .. import gemm_mx6
from .layers import ParamLinear

FLAG = "--mxfp6-linears"


def _blocks(module):
    return [b for _, b in module.named_modules() if hasattr(b, "hybrid_seq_parallel_attn") and hasattr(b, "run")]


def _gemm_linears(block):
    """the Linears of a block that run through models._gemm (the modulation Linears, M = 1, do not and stay bf16)"""
    if hasattr(block, "linear1"):
        return [block.linear1, block.linear2]
    return [l for s in ("img", "txt") for l in (getattr(block, f"{s}_attn_qkv"), getattr(block, f"{s}_attn_proj"),
                                                getattr(block, f"{s}_mlp").fc1, getattr(block, f"{s}_mlp").fc2)]


def convert_mxfp6_linear(module) -> int:
    """Pack qkv / proj / fc1 / fc2 per stream of every double block and linear1 / linear2 of every single block: layer.weight becomes the
    uint8 codes [out, 3 in / 4], layer.mx_scale the uint8 scales [out, in / 32]; the bf16 weight is released.  A layer has ONE stored
    format: a model converted by convert_fp8_linear or convert_mxfp4_linear is refused.  Returns the number of layers packed."""
    if getattr(module, "fp8_matmul_enabled", False):
        raise ValueError(f"{FLAG} and --use-fp8 exclude each other: a layer has one stored format (convert_fp8_linear already ran)")
    if getattr(module, "mxfp4_linears_converted", False):
        raise ValueError(f"{FLAG} and --mxfp4-linears exclude each other: a layer has one stored format (convert_mxfp4_linear already ran)")
    n = 0
    for block in _blocks(module):
        for layer in _gemm_linears(block):
            assert isinstance(layer, ParamLinear)
            if hasattr(layer, "mx_scale"):
                continue
            codes, scales = gemm_mx6.quant_rows_mxfp6(layer.weight.data)
            layer.weight = torch.nn.Parameter(codes, requires_grad=False)
            layer.mx_scale = scales
            layer.mx_format = 6          # what tells these uint8 codes from MXFP4 ones (models._linear_mode)
            n += 1
    module.mxfp6_linears_converted = True
    return n


def enable_mxfp6_linears(module, enable: bool = True) -> int:
    """Set the block flag models._ln / models._gemm test; a flagged block whose Linears are not packed keeps its bf16 path.  With
    sequence parallelism a flagged, packed block raises NotImplementedError (the chunked QKV slices weight rows).  Returns the
    number of blocks."""
    blocks = _blocks(module)
    for b in blocks:
        b.mxfp6_linears = bool(enable)
    return len(blocks)
