"""The tile geometry of the reference's AutoencoderKLCausal3D (autoencoder_kl_causal_3d.py:117-132, 362-541), once, for both halves
and both axis kinds.  Decode tiles the latent (source) and blends in sample space (output); encode is the same plan with the two
swapped.  Pure slicing and integer arithmetic on [C,T,H,W] views: no kernels, no GPU.

`TilePlan.temporal_tiles` / `spatial_rows` are the loops the assemblers of AutoencoderKLCausal3D walk, and `TilePlan.views` walks
the same two, so the tiles decoded ahead (two streams, tile-parallel ranks) come in the order the blends consume them by
construction."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple


@dataclass(frozen=True)
class AxisPlan:
    size: int          # source tile size (tile_latent_min_* for decode, tile_sample_min_* for encode)
    stride: int        # source distance between tile origins
    extent: int        # output positions blended with the previous tile
    limit: int         # output positions a tile contributes after the blend

    @classmethod
    def of(cls, size: int, out_size: int, overlap: float) -> "AxisPlan":
        extent = int(out_size * overlap)
        return cls(size, int(size * (1 - overlap)), extent, out_size - extent)

    def starts(self, n: int) -> range:
        return range(0, n, self.stride)


@dataclass(frozen=True)
class TilePlan:
    temporal: Optional[AxisPlan]          # None: that kind of tiling is switched off
    spatial: Optional[AxisPlan]

    def temporal_tiles(self, x4):
        """The temporal tiles of x4, each one frame longer than the tile size (the causal convs need the frame before), or None
        where x4 is not tiled in time."""
        t = self.temporal
        if t is None or x4.shape[1] <= t.size:
            return None
        return [x4[:, i:i + t.size + 1] for i in t.starts(x4.shape[1])]

    def temporal_frames(self, i: int) -> Tuple[int, int]:
        """(first, most) for the i-th temporal tile's output: every tile after the first drops its frame 0 (the previous tile's
        last frame, coded again) before the blend; `most` frames of what is left go to the result: limit + 1 for the first tile."""
        first = min(i, 1)
        return first, self.temporal.limit + 1 - first

    def spatial_rows(self, x4):
        """The spatial tiles of x4 as rows of columns, or None where x4 is not tiled in space."""
        s = self.spatial
        if s is None or (x4.shape[-1] <= s.size and x4.shape[-2] <= s.size):
            return None
        return [[x4[:, :, i:i + s.size, j:j + s.size] for j in s.starts(x4.shape[-1])] for i in s.starts(x4.shape[-2])]

    def views(self, x4):
        """Every tile the coder is called on, in the order the assemblers call it."""
        for group in self.temporal_tiles(x4) or [x4]:
            for row in self.spatial_rows(group) or [[group]]:
                yield from row


# ----------------------------------------------------------------------------------------------------------------------------------
# Frame counts under the fork's temporal ops (t_ops_config.json; unet_causal_3d_blocks.py:622-672,736-790,853-912).  The tile geometry
# above never looks at T while only space is tiled, but the tiles decoded ahead of the blends are sized before they exist, and with
# t_ops the decoder no longer gives 4 (T - 1) + 1 frames.  Pure integers, the walk of AutoencoderKLCausal3D._encode_tile / _decode_tile.

# per block, in each half's own order: (resamples H and W, resamples T) for the 884 ratios (AutoencoderKLCausal3D._resample_schedule)
SCHEDULE_884 = ((True, False), (True, True), (True, True), (False, False))


def _block_cfg(cfgs, i):
    for c in cfgs or []:
        if c.get("block_index") == i:
            return c
    return None


def _pooled(T: int, cfg, n_res: int) -> int:
    """T after the pools around the `n_res` resnets of one block: replicate-pad k - 1 frames in front, average k, stride s."""
    if not cfg or "enable_t_pool_before_block" not in cfg:
        return T
    s = int(cfg.get("pool_t_stride", 2))
    n = sum(bool(v) for v in cfg.get("enable_t_pool_before_block", [])[:n_res]) + \
        sum(bool(v) for v in cfg.get("enable_t_pool_after_block", [])[:n_res])
    for _ in range(n):
        T = (T - 1) // s + 1
    return T


def downsample_strides(t_ops=None, schedule=SCHEDULE_884):
    """Per encoder block: the (t, h, w) stride of its downsampler with the config's `downsample_stride` override applied, or None
    where the block has no downsampler (an override there is ignored, as in the reference)."""
    enc = (t_ops or {}).get("encoder", {})
    out = []
    for i, (sp, tm) in enumerate(schedule):
        if not (sp or tm):
            out.append(None)
            continue
        bc = _block_cfg(enc.get("down_blocks"), i)
        own = ((2 if tm else 1), (2 if sp else 1), (2 if sp else 1))
        out.append(tuple(int(v) for v in bc["downsample_stride"]) if bc and "downsample_stride" in bc else own)
    return out


def spatial_stride_overrides(t_ops=None, schedule=SCHEDULE_884):
    """Encoder blocks whose `downsample_stride` moves a spatial stride away from the schedule's own: [(block, (t, h, w)), ...]."""
    return [(i, st) for i, ((sp, tm), st) in enumerate(zip(schedule, downsample_strides(t_ops, schedule)))
            if st is not None and tuple(st[1:]) != ((2 if sp else 1),) * 2]


def encoded_frames(T: int, t_ops=None, schedule=SCHEDULE_884, layers_per_block: int = 2) -> int:
    """Latent frames the encoder gives for a clip of T frames: (T - 1) // 4 + 1 without t_ops."""
    enc = (t_ops or {}).get("encoder", {})
    for i, st in enumerate(downsample_strides(t_ops, schedule)):
        T = _pooled(T, _block_cfg(enc.get("down_blocks"), i), layers_per_block)
        if st is not None:
            T = (T - 1) // st[0] + 1
    return _pooled(T, enc.get("mid_block"), 2)


def decoded_frames(T: int, t_ops=None, schedule=SCHEDULE_884, layers_per_block: int = 2) -> int:
    """Frames the decoder gives for a latent of T frames: 4 (T - 1) + 1 without t_ops."""
    dec = (t_ops or {}).get("decoder", {})
    T = _pooled(T, dec.get("mid_block"), 2)
    for i, (sp, tm) in enumerate(schedule):
        bc = _block_cfg(dec.get("up_blocks"), i) or {}
        n = sum(bool(v) for v in bc.get("enable_t_interp_before_block", [])[:layers_per_block + 1]) + \
            sum(bool(v) for v in bc.get("enable_t_interp_after_block", [])[:layers_per_block + 1])
        T *= int(bc.get("interp_t_scale_factor", 2)) ** n
        if tm:
            T = 2 * T - 1
    return T
