"""Sliding-tile attention (include/hv_attn_tile.h, csrc/hv_attn_tile.hip; opt-in), public as ops.tile_plan, ops.TilePlan and
ops.attn_fwd_tile, and the switch enable_sliding_tile_attention.  The plan is index arithmetic on the host (torch integer ops, validated
before it reaches the device: the kernel trusts it like a pointer); the attention is the HIP kernel, GPU tensors only."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import _abi, _lib

ATTN_TILE = _abi.ATTN_TILE_MACROS     # HV_ATTN_TILE_BM / _KVT / _RING of include/hv_attn_tile.h


@dataclass(frozen=True)
class TilePlan:
    """the tile plan of include/hv_attn_tile.h: four int32 device tensors and what they describe"""
    perm: torch.Tensor          # [n_img] token row of each slot of the tile-ordered sequence
    tile_start: torch.Tensor    # [n_tiles + 1]
    nb_ptr: torch.Tensor        # [n_lists, n_tiles + 1]
    nb_idx: torch.Tensor        # [nnz]
    n_img: int
    n_tiles: int
    n_lists: int
    fraction: float             # attended (query, image key) pairs over n_img^2, the mean over the lists
    grid: Tuple[int, int, int]
    tile: Tuple[int, int, int]
    windows: Tuple[Tuple[int, int, int], ...]


def window_start(n_tiles: int, w: int) -> torch.Tensor:
    """first tile of the window of every tile along one axis: min(w, n_tiles) tiles centred on the tile (w // 2 before it), the centre
    clamped so that the window stays inside [0, n_tiles)"""
    return (torch.arange(n_tiles) - w // 2).clamp(0, n_tiles - min(w, n_tiles))


def tile_plan(grid: Sequence[int], tile: Sequence[int], window, device) -> TilePlan:
    """grid (T, H, W): the image tokens in (t, h, w) raster order; tile (tt, th, tw) <= 256 tokens; window (wt, wh, ww) in tiles, or one
    such triple per head.  Tiles partition the grid in raster order of tiles, edge tiles ragged; within a tile the tokens keep their
    raster order.  Every tile attends prod(min(w, tiles along the axis)) tiles, in raster order."""
    grid, tile = tuple(int(x) for x in grid), tuple(int(x) for x in tile)
    windows = [tuple(window)] if not isinstance(window[0], (tuple, list)) else [tuple(w) for w in window]
    windows = tuple(tuple(int(x) for x in w) for w in windows)
    if len(grid) != 3 or len(tile) != 3 or min(grid) < 1 or min(tile) < 1:
        raise ValueError(f"tile_plan: grid {grid} and tile {tile} must be three positive extents")
    if tile[0] * tile[1] * tile[2] > ATTN_TILE["HV_ATTN_TILE_BM"]:
        raise ValueError(f"tile_plan: a tile of {tile} holds {tile[0] * tile[1] * tile[2]} tokens, the kernel takes at most "
                         f"{ATTN_TILE['HV_ATTN_TILE_BM']} (HV_ATTN_TILE_BM)")
    if any(len(w) != 3 or min(w) < 1 for w in windows):
        raise ValueError(f"tile_plan: every window must be three entries >= 1, got {windows}")
    nt = tuple(-(-g // t) for g, t in zip(grid, tile))
    n_img, n_tiles = grid[0] * grid[1] * grid[2], nt[0] * nt[1] * nt[2]
    ax = [torch.arange(g) // t for g, t in zip(grid, tile)]
    tile_of = ((ax[0][:, None, None] * nt[1] + ax[1][None, :, None]) * nt[2] + ax[2][None, None, :]).reshape(-1)
    perm = torch.argsort(tile_of, stable=True)
    counts = torch.bincount(tile_of, minlength=n_tiles)
    tile_start = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    ptrs, idxs, pairs = [], [], 0
    for w in windows:
        lo = [window_start(n, x) for n, x in zip(nt, w)]
        span = [torch.arange(min(x, n)) for n, x in zip(nt, w)]
        a = (lo[0][:, None] + span[0][None, :])[:, None, None, :, None, None]
        b = (lo[1][:, None] + span[1][None, :])[None, :, None, None, :, None]
        c = (lo[2][:, None] + span[2][None, :])[None, None, :, None, None, :]
        nb = ((a * nt[1] + b) * nt[2] + c).reshape(n_tiles, -1)
        ptrs.append(torch.arange(n_tiles + 1) * nb.shape[1] + sum(i.numel() for i in idxs))
        idxs.append(nb.reshape(-1))
        pairs += int((counts[nb].sum(1) * counts).sum())
    nb_ptr, nb_idx = torch.stack(ptrs), torch.cat(idxs)
    # the kernel trusts these arrays: hold them to the header's rules before they leave the host
    if not (torch.equal(perm.sort().values, torch.arange(n_img)) and int(counts.min()) >= 1 and
            int(counts.max()) <= ATTN_TILE["HV_ATTN_TILE_BM"] and int(tile_start[-1]) == n_img and
            int(nb_idx.min()) >= 0 and int(nb_idx.max()) < n_tiles and bool((nb_ptr[:, 1:] >= nb_ptr[:, :-1]).all()) and
            int(nb_ptr.min()) >= 0 and int(nb_ptr.max()) <= nb_idx.numel() < 2 ** 31):
        raise AssertionError(f"tile_plan: grid {grid}, tile {tile}, windows {windows} gave an invalid plan")
    dev = lambda t: t.to(torch.int32).contiguous().to(device)
    return TilePlan(dev(perm), dev(tile_start), dev(nb_ptr), dev(nb_idx), n_img, n_tiles, len(windows),
                    pairs / (len(windows) * float(n_img) ** 2), grid, tile, windows)


def attn_fwd_tile(q, k, v, out, n_heads: int, plan: TilePlan, dense=(0, 0), scale: Optional[float] = None):
    """hv_attn_fwd_tile_bf16: q [n_img, >= H*128], k, v [n_kv, ..], out [n_img, ..] 2-D bf16 views (head h at column h*128).  Query slot
    s is token row plan.perm[s]; its keys are the rows of its tile's neighbour tiles and the rows [dense[0], dense[1]) of k, v."""
    from .ops import BF16, _chk
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out")):
        _chk(t, BF16, nm)
        assert t.dim() == 2
    n_q, n_kv = q.shape[0], k.shape[0]
    assert v.shape[0] == n_kv and out.shape[0] == n_q
    if plan.n_img != n_q:
        raise ValueError(f"attn_fwd_tile: the plan is for {plan.n_img} image tokens, q has {n_q} rows")
    if plan.perm.device != q.device:
        raise ValueError(f"attn_fwd_tile: the plan is on {plan.perm.device}, q on {q.device}")
    if plan.n_lists not in (1, n_heads):
        raise ValueError(f"attn_fwd_tile: the plan has {plan.n_lists} window lists for {n_heads} heads")
    _lib.call("attn_fwd_tile_bf16", q, k, v, out, q.stride(0), k.stride(0), v.stride(0), out.stride(0), n_q, n_kv, n_heads, 128,
              128 ** -0.5 if scale is None else scale, plan.perm, plan.tile_start, plan.n_tiles, plan.nb_ptr, plan.nb_idx, plan.n_lists,
              int(dense[0]), int(dense[1]))
    return out


def enable_sliding_tile_attention(model, tile=(4, 8, 8), window=(3, 3, 3), enable: bool = True) -> int:
    """Opt-in SLIDING-TILE attention: every double / single block attends, for an image query, only the tiles of `window` around its own
    tile plus all valid text (ops.attn_fwd_tile); text queries still attend everything; the padding segment is unchanged.  `window` is one
    triple or one per head.  The default tile (4, 8, 8) makes a full tile one 256-row workgroup and four full key chunks.  An
    approximation of the model, not the reference's arithmetic; no fidelity of generated video has been measured under any window.
    Together with sequence parallelism or fp8_attention the blocks raise NotImplementedError.  Returns the number of blocks."""
    if enable and getattr(model, "adaptive_tile", None) is not None:
        raise ValueError("enable_sliding_tile_attention: enable_adaptive_tile_attention (attn_select.py) is on for this model; a block "
                         "has one source of key-tile lists: switch that one off first")
    n = 0
    for _, block in model.named_modules():
        if hasattr(block, "hybrid_seq_parallel_attn") and hasattr(block, "run"):
            block.sliding_tile = bool(enable)
            n += 1
    model.sliding_tile = (tuple(tile), window) if enable else None
    model._tile_plans = {}
    return n


def model_plan(model, grid, device) -> Optional[TilePlan]:
    """the plan of a model under enable_sliding_tile_attention for this token grid, cached per (grid, tile, window, device)"""
    cfg = getattr(model, "sliding_tile", None)
    if cfg is None:
        return None
    key = (tuple(grid), cfg[0], str(cfg[1]), str(device))
    if key not in model._tile_plans:
        model._tile_plans[key] = tile_plan(grid, cfg[0], cfg[1], device)
    return model._tile_plans[key]
