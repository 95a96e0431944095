"""MXFP4 linears (opt-in; include/hv_gemm_mx4.h): pack the block GEMM weights as e2m1 codes + E8M0 block scales and run them, with
activations quantised the same way, on v_mfma_scale_f32_16x16x128_f8f6f4.  Not the reference's arithmetic: round-to-nearest e2m1 on both
operands carries roughly 10 % relative noise per element.  convert_mxfp4_linear(rot=16 / 64 / 256) rotates both operands by a
block-diagonal Hadamard matrix along K (include/hv_mx_rot.h), which spreads outlier channels over their group and changes nothing on
Gaussian data.  convert_mxfp4_linear(lowrank=32 / 64 / 96 / 128) splits W = Up Dn + Res by an SVD, packs only Res and multiplies the
rank-R part in bf16 from the unquantised activations (include/hv_mx_lowrank.h), which removes the error of a weight's dominant directions
(about ninefold on a weight with a strong rank-4 part, by the share of the spectrum R directions carry on a Gaussian one).  Nothing here
calibrates on data, and no run on real weights has measured video fidelity under any of these forms."""
from __future__ import annotations

import torch

from .. import gemm_mx4, mx_lowrank, mx_rot
from .layers import ParamLinear

FLAG = "--mxfp4-linears"


def _blocks(module):
    return [b for _, b in module.named_modules() if hasattr(b, "hybrid_seq_parallel_attn") and hasattr(b, "run")]


def _gemm_linears(block):
    """the Linears of a block that run through models._gemm (the modulation Linears, M = 1, do not and stay bf16)"""
    if hasattr(block, "linear1"):
        return [block.linear1, block.linear2]
    return [l for s in ("img", "txt") for l in (getattr(block, f"{s}_attn_qkv"), getattr(block, f"{s}_attn_proj"),
                                                getattr(block, f"{s}_mlp").fc1, getattr(block, f"{s}_mlp").fc2)]


def convert_mxfp4_linear(module, rot: int = 0, lowrank: int = 0) -> int:
    """Pack qkv / proj / fc1 / fc2 per stream of every double block and linear1 / linear2 of every single block: layer.weight becomes the
    uint8 codes [out, in / 2], layer.mx_scale the uint8 scales [out, in / 32]; the bf16 weight is released.  A layer has ONE stored
    format: a model converted by convert_fp8_linear is refused.  rot > 0 (16, 64 or 256) packs W H instead of W, H the block-diagonal
    Hadamard rotation of include/hv_mx_rot.h, and records layer.mx_rot: models._ln / models._gemm then quantise the layer's activations
    through the rotated quantisers, (A H)(W H)^T = A W^T.  lowrank > 0 (32, 64, 96 or 128) packs Res of W = Up Dn + Res
    (mx_lowrank.factorise: a deterministic fp32 SVD per layer) and stores layer.mx_lr_up [out, R], layer.mx_lr_dn [R, in] and
    layer.mx_lowrank: models._gemm then runs the layer through the two kernels of include/hv_mx_lowrank.h.  rot and lowrank together
    are not built.  Returns the number of layers packed."""
    if lowrank not in (0,) + mx_lowrank.RANKS:
        raise ValueError(f"lowrank must be 0 or one of {mx_lowrank.RANKS}, got {lowrank}")
    if rot and lowrank:
        raise ValueError("rot > 0 together with lowrank > 0 is not built: the down-projection would have to read the unrotated rows")
    if rot not in (0,) + mx_rot.ROTS:
        raise ValueError(f"rot must be 0 or one of {mx_rot.ROTS}, got {rot}")
    if getattr(module, "fp8_matmul_enabled", False):
        raise ValueError(f"{FLAG} and --use-fp8 exclude each other: a layer has one stored format (convert_fp8_linear already ran)")
    if getattr(module, "mxfp6_linears_converted", False):
        raise ValueError(f"{FLAG} and --mxfp6-linears exclude each other: a layer has one stored format (convert_mxfp6_linear already ran)")
    layers = [l for block in _blocks(module) for l in _gemm_linears(block) if not hasattr(l, "mx_scale")]
    for layer in layers:                    # refuse before the first layer is packed
        assert isinstance(layer, ParamLinear)
        if rot and layer.in_features % rot:
            raise ValueError(f"rot = {rot} does not divide in_features = {layer.in_features}: rotation groups are whole")
    for layer in layers:
        w = layer.weight.data
        if lowrank:
            layer.mx_lr_up, layer.mx_lr_dn, w = mx_lowrank.factorise(w, lowrank)
        codes, scales = mx_rot.quant_rows_mxfp4_rot(w, rot) if rot else gemm_mx4.quant_rows_mxfp4(w)
        layer.weight = torch.nn.Parameter(codes, requires_grad=False)
        layer.mx_scale = scales
        layer.mx_rot = rot
        layer.mx_lowrank = lowrank
    module.mxfp4_linears_converted = True
    return len(layers)


def enable_mxfp4_linears(module, enable: bool = True) -> int:
    """Set the block flag models._ln / models._gemm test; a flagged block whose Linears are not packed keeps its bf16 path.  With
    sequence parallelism a flagged, packed block raises NotImplementedError (the chunked QKV slices weight rows).  Returns the
    number of blocks."""
    blocks = _blocks(module)
    for b in blocks:
        b.mxfp4_linears = bool(enable)
    return len(blocks)
