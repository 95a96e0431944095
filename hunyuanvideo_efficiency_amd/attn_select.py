"""Adaptive tile attention (include/hv_attn_select.h, csrc/hv_attn_select.hip; opt-in): the key-tile lists of ops.attn_fwd_tile chosen
on the GPU, per call and per head, from the pooled Q.K of that call.  select_plan turns a base TilePlan (its perm and tile boundaries) into
a TilePlan whose nb_ptr / nb_idx the kernels wrote; nothing is read back.  Public HERE, not re-exported through ops (no CPU double;
tests/attn_select_ref.py restates the rule for the GPU tests); the attention itself goes through ops.attn_fwd_tile."""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import _abi, _lib
from .attn_tile import TilePlan, tile_plan

ATTN_SELECT = _abi.ATTN_SELECT_MACROS     # HV_ATTN_SELECT_MAX_TILES / _BAND of include/hv_attn_select.h
MAX_TILES = ATTN_SELECT["HV_ATTN_SELECT_MAX_TILES"]


def select_buffers(n_tiles: int, n_heads: int, k_max: Optional[int], device, kept_mass: bool = False) -> dict:
    """the caller-owned outputs and workspace of hv_attn_select_tiles for this shape: nb_idx holds n_heads * n_tiles * min(k_max,
    n_tiles) entries (k_max None: every tile), whatever the lists turn out to need"""
    need = _lib.host("attn_select_workspace_bytes", n_tiles, n_heads)
    if need <= 0:
        raise ValueError(f"select_buffers: {n_tiles} tiles (at most {MAX_TILES}) x {n_heads} heads is not a shape the selection takes")
    cap = n_heads * n_tiles * min(n_tiles if k_max is None else int(k_max), n_tiles)
    i32 = dict(dtype=torch.int32, device=device)
    return dict(nb_ptr=torch.empty(n_heads, n_tiles + 1, **i32), nb_idx=torch.empty(max(cap, 1), **i32),
                workspace=torch.empty(need, dtype=torch.uint8, device=device),
                kept_mass=torch.empty(n_heads, n_tiles, dtype=torch.float32, device=device) if kept_mass else None)


def select_plan(q, k, n_heads: int, base: TilePlan, cdf: float = 0.9, k_min: int = 1, k_max: Optional[int] = None,
                scale: Optional[float] = None, buffers: Optional[dict] = None) -> TilePlan:
    """hv_attn_select_tiles: q, k [n_img, >= H*128] 2-D bf16 views (head h at column h*128; the image rows of the fused QKV buffer) ->
    `base` with per-head key-tile lists: tile i of head h keeps the shortest prefix of its key tiles, ranked by pooled softmax mass with
    its own tile first, that reaches `cdf`, clamped to [k_min, k_max] tiles.  `buffers` (select_buffers) are reused when given: the
    returned plan aliases them, so a plan is valid until the next call with the same buffers.  fraction is NaN: reading it would
    synchronise (plan_density does, on request)."""
    from .ops import BF16, _chk
    for t, nm in ((q, "q"), (k, "k")):
        _chk(t, BF16, nm)
        assert t.dim() == 2 and t.shape[0] == base.n_img and t.shape[1] >= n_heads * 128, (nm, t.shape, base.n_img, n_heads)
    if base.perm.device != q.device:
        raise ValueError(f"select_plan: the plan is on {base.perm.device}, q on {q.device}")
    kmax = base.n_tiles if k_max is None else int(k_max)
    if not (0.0 < cdf <= 1.0) or not (1 <= k_min <= kmax):
        raise ValueError(f"select_plan: cdf must lie in (0, 1] and 1 <= k_min <= k_max, got cdf={cdf}, k_min={k_min}, k_max={k_max}")
    b = select_buffers(base.n_tiles, n_heads, k_max, q.device) if buffers is None else buffers
    if tuple(b["nb_ptr"].shape) != (n_heads, base.n_tiles + 1):
        raise ValueError(f"select_plan: the buffers are for nb_ptr {tuple(b['nb_ptr'].shape)}, this call needs {(n_heads, base.n_tiles + 1)}")
    _lib.call("attn_select_tiles", q, k, q.stride(0), k.stride(0), base.n_img, n_heads, 128, 128 ** -0.5 if scale is None else scale,
              base.perm, base.tile_start, base.n_tiles, float(cdf), int(k_min), kmax, b["nb_ptr"], b["nb_idx"], b["nb_idx"].numel(),
              b["kept_mass"], b["workspace"], b["workspace"].numel())
    return dataclasses.replace(base, nb_ptr=b["nb_ptr"], nb_idx=b["nb_idx"], n_lists=n_heads, fraction=float("nan"), windows=())


def plan_density(plan: TilePlan) -> float:
    """attended (query, image key) pairs over n_img^2, the mean over the plan's lists - read back from the device (synchronises)"""
    c, ptr = plan.tile_start.long().diff(), plan.nb_ptr.long()
    lens = (ptr[:, 1:] - ptr[:, :-1]).reshape(-1)
    idx = plan.nb_idx[int(ptr[0, 0]):int(ptr[-1, -1])].long()
    per_entry = torch.repeat_interleave(c.repeat(plan.n_lists), lens) * c[idx]
    return float(per_entry.sum()) / (plan.n_lists * float(plan.n_img) ** 2)


def enable_adaptive_tile_attention(model, tile=(4, 8, 8), cdf: float = 0.9, k_min: int = 1, k_max: Optional[int] = None,
                                   enable: bool = True) -> int:
    """Opt-in ADAPTIVE TILE attention: every double / single block runs select_plan on its own q and k and then ops.attn_fwd_tile under
    the lists it got: an image query attends the key tiles that carry `cdf` of its tile's pooled softmax mass (at least k_min, at most
    k_max tiles, its own always) plus all valid text; text queries still attend everything; the padding segment is unchanged.  An
    approximation of the model; no fidelity of generated video has been measured under any setting.  Together with sequence parallelism
    or fp8_attention the blocks raise NotImplementedError; together with enable_sliding_tile_attention it is a ValueError.  Returns the
    number of blocks."""
    if enable and getattr(model, "sliding_tile", None) is not None:
        raise ValueError("enable_adaptive_tile_attention: enable_sliding_tile_attention is on for this model; a block has one source of "
                         "key-tile lists: switch that one off first")
    if enable and (not (0.0 < cdf <= 1.0) or k_min < 1 or (k_max is not None and k_max < k_min)):
        raise ValueError(f"enable_adaptive_tile_attention: cdf must lie in (0, 1] and 1 <= k_min <= k_max, got {cdf}, {k_min}, {k_max}")
    n = 0
    for _, block in model.named_modules():
        if hasattr(block, "hybrid_seq_parallel_attn") and hasattr(block, "run"):
            block.adaptive_tile = bool(enable)
            n += 1
    model.adaptive_tile = dict(tile=tuple(tile), cdf=float(cdf), k_min=int(k_min), k_max=k_max) if enable else None
    model._adaptive_states = {}
    return n


@dataclasses.dataclass
class AdaptiveState:
    """what a forward under enable_adaptive_tile_attention keeps per token grid: the base plan and one set of buffers every block reuses"""
    base: TilePlan
    buffers: dict
    cdf: float
    k_min: int
    k_max: Optional[int]

    def select(self, q, k, n_heads: int) -> TilePlan:
        return select_plan(q, k, n_heads, self.base, self.cdf, min(self.k_min, self.base.n_tiles), self.k_max, buffers=self.buffers)


def model_state(model, grid, n_heads: int, device) -> Optional[AdaptiveState]:
    """the AdaptiveState of a model under enable_adaptive_tile_attention for this token grid, cached per (grid, heads, device)"""
    cfg = getattr(model, "adaptive_tile", None)
    if cfg is None:
        return None
    key = (tuple(grid), n_heads, str(device))
    if key not in model._adaptive_states:
        base = tile_plan(grid, cfg["tile"], (1, 1, 1), device)          # perm and tile boundaries; its one-tile lists are not used
        if base.n_tiles > MAX_TILES:
            raise ValueError(f"adaptive tile attention: grid {tuple(grid)} in tiles of {cfg['tile']} has {base.n_tiles} tiles, the "
                             f"selection takes at most {MAX_TILES} (HV_ATTN_SELECT_MAX_TILES): choose a larger tile")
        model._adaptive_states[key] = AdaptiveState(base, select_buffers(base.n_tiles, n_heads, cfg["k_max"], device), cfg["cdf"],
                                                    cfg["k_min"], cfg["k_max"])
    return model._adaptive_states[key]
