"""ORACLE-side restatement (test infrastructure) of the reference's two spatial tile loops (autoencoder_kl_causal_3d.py:362-469) with the
tile coder passed in, so that a tile can be encoded / decoded under a t_ops configuration: oracle/vae_enc_ref.spatial_tiled_encode and
oracle/vae_ref's tiled decode call the plain coders.  Pinned by tests/golden/vae_tinterp.npz (the reference's own loops run with t_ops
applied to its encoder and decoder) in tests/test_oracle_vae_tinterp_golden.py."""
from __future__ import annotations

import torch

from oracle import vae_enc_ref as E
from oracle.vae_ref import Prec, TileParams, _blend


def _tiled(x, coder, src_size: int, out_size: int, overlap: float, p: Prec):
    ov = int(src_size * (1 - overlap))
    ext = int(out_size * overlap)
    lim = out_size - ext
    rows = [[coder(x[..., i:i + src_size, j:j + src_size]) for j in range(0, x.shape[-1], ov)] for i in range(0, x.shape[-2], ov)]
    out_rows = []
    for i, row in enumerate(rows):
        res = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = _blend(rows[i - 1][j], tile, ext, 3, p)
            if j > 0:
                tile = _blend(row[j - 1], tile, ext, 4, p)
            res.append(tile[..., :lim, :lim])
        out_rows.append(torch.cat(res, dim=-1))
    return torch.cat(out_rows, dim=-2)


def spatial_tiled_encode(sd, x, boc, tp: TileParams, p: Prec, t_ops=None):
    """-> moments; every tile through encode_tile(..., t_ops)"""
    return _tiled(x, lambda v: E.encode_tile(sd, v, boc, p, t_ops), tp.tile_sample_min_size, tp.tile_latent_min_size,
                  tp.tile_overlap_factor, p)


def spatial_tiled_decode(sd, z, boc, tp: TileParams, p: Prec, t_ops=None):
    """-> sample; every tile through decode_tile_tops(..., t_ops)"""
    return _tiled(z, lambda v: E.decode_tile_tops(sd, v, boc, p, t_ops), tp.tile_latent_min_size, tp.tile_sample_min_size,
                  tp.tile_overlap_factor, p)
