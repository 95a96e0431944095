"""The VAE's tile geometry on the CPU, exactly: the assembled result of the product's tiling loops (tile order, +1 temporal frame,
dropped first frames, blend-above / blend-left / crop-copy, temporal blend then copy) against the oracle's restatement of the
reference's loops (oracle/vae_ref.py, oracle/vae_enc_ref.py), with the same deterministic stand-in for the tile decoder / encoder on
both sides and the oracle's own `_blend` as the blend kernel's double.  Both sides then do the same fp16 arithmetic on the same
values, so the comparison has no tolerance; the GPU tests compare the real kernels against goldens with a 30-layer fp16 bound that
a mis-ordered blend of similar tiles could hide in."""
import pytest
import torch

from hunyuanvideo_efficiency_amd import vae_ops
from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D
from oracle import vae_enc_ref as EO
from oracle import vae_ref as R

F16 = torch.float16
E = R.Prec(True)
LATENT = 16

# (sample_size, sample_tsize, latent shape, decode tiles with temporal+spatial / spatial / temporal / no tiling)
CASES = [
    (32, 8, (1, 16, 4, 7, 6), (24, 6, 4, 1)),        # the golden's shape: ragged spatial edge, 4 temporal tiles
    (32, 8, (1, 16, 1, 9, 4), (6, 6, 1, 1)),         # a single frame: spatial tiling only
    (64, 16, (1, 16, 6, 14, 12), (12, 6, 2, 1)),
    (32, 8, (1, 16, 5, 4, 11), (40, 8, 5, 1)),       # a trailing temporal tile of one latent frame
    (32, 8, (1, 16, 2, 3, 3), (1, 1, 1, 1)),         # nothing tiles
]
TILING = [(True, True), (False, True), (True, False), (False, False)]      # (temporal, spatial), in the order of the counts above


def _fake_planar(x, c_out, T, H, W):
    """Stand-in tile coder: planar fp16-representable [c_out,T,H,W], a fixed function of position plus a term from the sum of the
    input view (exact: the inputs are small multiples of 1/64), so tiles of equal shape still differ."""
    c, t, h, w = torch.meshgrid(torch.arange(c_out), torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
    pos = ((c * 37 + t * 11 + h * 5 + w * 3) % 61).float() / 64.0 - 0.5
    term = float(torch.round(x.double().sum() * 64.0)) % 97.0 / 128.0
    return (pos + term).to(F16).float()


def _fake_decode_planar(z):
    T, H, W = (z.shape[-3] - 1) * 4 + 1, z.shape[-2] * 8, z.shape[-1] * 8
    return _fake_planar(z, 3, T, H, W)


def _fake_encode_planar(x):
    T, H, W = (x.shape[-3] - 1) // 4 + 1, x.shape[-2] // 8, x.shape[-1] // 8
    return _fake_planar(x, 2 * LATENT, T, H, W)


def _channels_last(planar, cols):
    c, T, H, W = planar.shape
    buf = torch.zeros(T * H * W, cols, dtype=F16)
    buf[:, :c] = planar.permute(1, 2, 3, 0).reshape(-1, c).to(F16)
    return buf, T, H, W


def _grid_values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32, 33, shape, generator=g).float() / 64.0


def _vae(monkeypatch, ss, ts, temporal, spatial):
    vae = AutoencoderKLCausal3D(block_out_channels=(32, 32, 32, 32), sample_size=ss, sample_tsize=ts, device="cpu",
                                with_encoder=True)
    vae.enable_temporal_tiling(temporal)
    vae.enable_spatial_tiling(spatial)
    monkeypatch.setattr(vae_ops, "blend_", lambda a, b, axis, extent: R._blend(a[None], b[None], extent, axis + 1, E)[0])
    monkeypatch.setattr(vae_ops, "copy4d_", lambda src, dst: dst.copy_(src))
    return vae


def _same_view(a, b):
    return a.shape == b.shape and a.stride() == b.stride() and a.storage_offset() == b.storage_offset() and torch.equal(a, b)


@pytest.mark.parametrize("tiling", TILING, ids=lambda t: "T%dS%d" % t)
@pytest.mark.parametrize("ss,ts,shape,counts", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tiled_decode_assembly_equals_oracle_loops(monkeypatch, ss, ts, shape, counts, tiling):
    temporal, spatial = tiling
    vae = _vae(monkeypatch, ss, ts, temporal, spatial)
    z = _grid_values(shape, 1)
    seen = []

    def fake_tile(z_view):
        seen.append(z_view)
        return _channels_last(_fake_decode_planar(z_view), 8)
    vae._decode_tile = fake_tile
    y = vae.decode(z, return_dict=False)[0]

    monkeypatch.setattr(R, "decode_tile", lambda sd, zt, boc, p: _fake_decode_planar(zt[0])[None])
    tp = R.TileParams(sample_size=ss, sample_tsize=ts, n_blocks=4)
    if temporal and z.shape[2] > tp.tile_latent_min_tsize:
        ref = R.temporal_tiled_decode(None, z, None, tp, E, spatial=spatial)
    elif spatial and (z.shape[-1] > tp.tile_latent_min_size or z.shape[-2] > tp.tile_latent_min_size):
        ref = R.spatial_tiled_decode(None, z, None, tp, E)
    else:
        ref = R.decode_tile(None, z, None, E)
    assert y.dtype == F16 and y.shape == ref.shape
    assert torch.equal(y.float(), ref)

    # the enumeration the tile-parallel and two-stream paths decode ahead from: the very tiles, in the very order, the loops consume
    views = list(vae._tile_views(z[0]))
    assert len(views) == len(seen) == counts[TILING.index(tiling)]
    assert all(_same_view(v, s) for v, s in zip(views, seen))

    # tiles decoded ahead (what the two-stream and the tile-parallel paths hand to the blends) assemble to the same bytes
    vae._decode_tiles_concurrent = lambda z4: [fake_tile(v) for v in vae._tile_views(z4)]
    assert torch.equal(vae.decode(z, return_dict=False)[0], y)


@pytest.mark.parametrize("tiling", TILING, ids=lambda t: "T%dS%d" % t)
@pytest.mark.parametrize("ss,ts,shape,counts", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tiled_encode_assembly_equals_oracle_loops(monkeypatch, ss, ts, shape, counts, tiling):
    temporal, spatial = tiling
    vae = _vae(monkeypatch, ss, ts, temporal, spatial)
    x = _grid_values((1, 3, (shape[2] - 1) * 4 + 1, shape[3] * 8, shape[4] * 8), 2)
    vae._encode_tile = lambda x_view: _channels_last(_fake_encode_planar(x_view), 2 * LATENT)
    m = vae.encode(x).latent_dist.parameters

    monkeypatch.setattr(EO, "encode_tile", lambda sd, xt, boc, p, t_ops=None: _fake_encode_planar(xt[0])[None])
    tp = R.TileParams(sample_size=ss, sample_tsize=ts, n_blocks=4)
    if temporal and x.shape[2] > tp.tile_sample_min_tsize:
        ref = EO.temporal_tiled_encode(None, x, None, tp, E, spatial=spatial)
    elif spatial and (x.shape[-1] > tp.tile_sample_min_size or x.shape[-2] > tp.tile_sample_min_size):
        ref = EO.spatial_tiled_encode(None, x, None, tp, E)
    else:
        ref = EO.encode_tile(None, x, None, E)
    assert m.dtype == F16 and m.shape == ref.shape
    assert torch.equal(m.float(), ref)
