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
