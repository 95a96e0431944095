#!/usr/bin/env python3
"""Generate tests/golden/vae_tinterp.npz by executing the reference's VAE code on CPU (fp32) under t_ops configurations that the
existing goldens do not reach: interp_mode "trilinear" in the decoder, and the reference's own spatial tile loops (spatial_tiled_encode,
spatial_tiled_decode) run with a t_ops configuration applied to the encoder and decoder they call.

Same loading recipe as tools/make_golden_vae_enc.py (whose stubs, method extraction and apply_t_ops it uses).  Inputs are fp16-valued
fp32 arrays, so the fp16 kernels see exactly what the reference saw.  The file holds data only: inputs, outputs, the two configurations
as JSON text, the tile sizes.
Run: python tools/make_golden_vae_tinterp.py"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
import make_golden_vae as G  # noqa: E402
import make_golden_vae_enc as GE  # noqa: E402

BOC = (32, 64, 128, 128)


def _up(i, before=(False,) * 3, after=(False,) * 3, sc=2, mode="trilinear"):
    return {"block_index": i, "enable_t_interp_before_block": list(before), "enable_t_interp_after_block": list(after),
            "interp_t_scale_factor": sc, "interp_mode": mode}


def _down(i, before=(False,) * 2, after=(False,) * 2, k=3, s=2):
    return {"block_index": i, "pool_t_kernel": k, "pool_t_stride": s, "enable_t_pool_before_block": list(before),
            "enable_t_pool_after_block": list(after)}


_NO_MID = {"enable_t_pool_before_block": [False, False], "enable_t_pool_after_block": [False, False]}
# decoder: trilinear x2 before resnet 1 of block 1 and x3 after resnet 2 of block 2 (an odd factor has a weight-0 frame per interval)
T_OPS_TRILINEAR = {
    "encoder": {"down_blocks": [_down(i) for i in range(4)], "mid_block": dict(_NO_MID, pool_t_kernel=3, pool_t_stride=2)},
    "decoder": {"up_blocks": [_up(0), _up(1, before=(False, True, False)), _up(2, after=(False, False, True), sc=3), _up(3)],
                "mid_block": dict(_NO_MID)},
}
# tiled in space: one pool (before resnet 1 of encoder block 0) and one trilinear interpolation (after resnet 0 of decoder block 2)
T_OPS_TILED = {
    "encoder": {"down_blocks": [_down(0, before=(False, True))] + [_down(i) for i in range(1, 4)],
                "mid_block": dict(_NO_MID, pool_t_kernel=3, pool_t_stride=2)},
    "decoder": {"up_blocks": [_up(0), _up(1), _up(2, after=(True, False, False)), _up(3)], "mid_block": dict(_NO_MID)},
}
TILE = dict(tile_sample_min_tsize=64, tile_latent_min_tsize=16, tile_sample_min_size=32, tile_latent_min_size=4, tile_overlap_factor=0.25)


def f16_valued(shape, key, scale=1.0):
    return (syn.hashed_uniform(shape, key, 1) * scale).half().float()


def build(V, t_ops):
    enc = V.EncoderCausal3D(in_channels=3, out_channels=16, down_block_types=("DownEncoderBlockCausal3D",) * 4,
                            block_out_channels=BOC, layers_per_block=2, norm_num_groups=32, act_fn="silu", double_z=True,
                            time_compression_ratio=4, spatial_compression_ratio=8, mid_block_add_attention=True)
    dec = V.DecoderCausal3D(in_channels=16, out_channels=3, up_block_types=("UpDecoderBlockCausal3D",) * 4,
                            block_out_channels=BOC, layers_per_block=2, norm_num_groups=32, act_fn="silu",
                            time_compression_ratio=4, spatial_compression_ratio=8, mid_block_add_attention=True)
    sd = syn.synth_vae_state_dict(BOC, seed=0, encoder=True)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=True)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")}, strict=True)
    enc.eval(), dec.eval()
    qc, pq = nn.Conv3d(32, 32, kernel_size=1), nn.Conv3d(16, 16, kernel_size=1)
    qc.weight.copy_(sd["quant_conv.weight"]), qc.bias.copy_(sd["quant_conv.bias"])
    pq.weight.copy_(sd["post_quant_conv.weight"]), pq.bias.copy_(sd["post_quant_conv.bias"])
    GE.apply_t_ops(enc, dec, t_ops)
    return enc, dec, qc, pq


def main():
    torch.set_grad_enabled(False)
    m = G.install_stubs()
    V = m["vae"]

    # ---- decoder with trilinear interpolations: latent [1,16,2,4,3] -> [1,3,41,32,24]   (T: 2 -> x2 = 4 -> 7 -> x3 = 21 -> 41)
    enc, dec, qc, pq = build(V, T_OPS_TRILINEAR)
    z = f16_valued((1, 16, 2, 4, 3), "gt.z", 1.7)
    y = dec(pq(z))
    print("trilinear decode:", tuple(z.shape), "->", tuple(y.shape))

    # ---- the reference's spatial tile loops under t_ops: 2 x 2 tiles, ragged last row and column, both halves
    enc, dec, qc, pq = build(V, T_OPS_TILED)
    methods = dict(GE.tiled_encode_methods(V.DiagonalGaussianDistribution))
    methods.update({k: v for k, v in G.tiling_methods().items() if k == "spatial_tiled_decode"})
    ae = types.SimpleNamespace(encoder=enc, decoder=dec, quant_conv=qc, post_quant_conv=pq, use_spatial_tiling=True,
                               use_temporal_tiling=False, **TILE)
    for n, f in methods.items():
        setattr(ae, n, types.MethodType(f, ae))
    x = f16_valued((1, 3, 9, 48, 40), "gt.video")
    moments = ae.spatial_tiled_encode(x, return_moments=True)
    zt = f16_valued((1, 16, 2, 6, 5), "gt.zt", 1.7)
    yt = ae.spatial_tiled_decode(zt, return_dict=True).sample
    print("tiled under t_ops: video", tuple(x.shape), "-> moments", tuple(moments.shape), "; latent", tuple(zt.shape), "->", tuple(yt.shape))

    enc_json = lambda c: np.frombuffer(json.dumps(c).encode(), dtype=np.uint8)
    G.save("vae_tinterp", z=z, y=y, t_ops_json=enc_json(T_OPS_TRILINEAR), x_tiled=x, moments_tiled=moments, z_tiled=zt, y_tiled=yt,
           t_ops_tiled_json=enc_json(T_OPS_TILED), tile=np.array([TILE["tile_sample_min_size"], TILE["tile_latent_min_size"]]),
           block_out_channels=np.array(BOC))


if __name__ == "__main__":
    main()
