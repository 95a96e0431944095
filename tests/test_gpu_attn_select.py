"""GPU: adaptive tile selection (include/hv_attn_select.h) against its float64 restatement, tests/attn_select_ref.py.
(1) the lists follow the rule wherever fp32 cannot decide a comparison at the cut otherwise, and are valid lists everywhere; (2) cdf = 1
gives the lists of a window over the whole grid, bit for bit, and the same attention output; (3) the lists drive the tile kernel inside
the dense kernel's fp64 bound (tests/attention_bounds.py); (4) the tiny model under the flag."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import attention_bounds as AB  # noqa: E402
from tests import attn_select_ref as R  # noqa: E402

DEV, D = "cuda", 128
GEOS = [((1, 2, 3), (1, 2, 3)),         # one tile
        ((3, 5, 9), (2, 2, 4)),         # 18 ragged tiles of 16 ... 1 slots
        ((1, 3, 33), (1, 3, 1)),        # 33 tiles: one past an MFMA block and a band
        ((3, 9, 22), (1, 3, 2)),        # 99 tiles: four bands, four key blocks, two bitmask word pairs
        ((5, 8, 16), (4, 8, 8))]        # 256-slot tiles beside 64-slot ones
PARAMS = [(0.5, 1, None), (0.9, 2, 5), (1.0, 1, 3), (1.0, 1, None)]
ids = lambda x: "-".join("x".join(map(str, t)) if isinstance(t, tuple) else str(t) for t in x)


@pytest.fixture(scope="module")
def sel():
    from hunyuanvideo_efficiency_amd import attn_select, _lib
    _lib.torch_ops()
    return attn_select


def on_gpu(base):
    return dataclasses.replace(base, **{f: getattr(base, f).to(DEV) for f in ("perm", "tile_start", "nb_ptr", "nb_idx")})


def run_select(sel, base, buf, H, cdf, k_min, k_max, guard=64):
    """select_plan into hand-made buffers with guard words behind nb_idx and the workspace -> plan, buffers, read-back lists per head"""
    nt = base.n_tiles
    b = sel.select_buffers(nt, H, k_max, DEV, kept_mass=True)
    cap, need = b["nb_idx"].numel(), b["workspace"].numel()
    idx_all, ws_all = torch.full((cap + guard,), -7, dtype=torch.int32, device=DEV), torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    b["nb_idx"], b["workspace"] = idx_all[:cap], ws_all[:need]
    gb = buf.to(DEV)
    plan = sel.select_plan(gb[:base.n_img, :H * D], gb[:base.n_img, H * D:2 * H * D], H, on_gpu(base), cdf, k_min, k_max, buffers=b)
    ptr, idx = plan.nb_ptr.cpu(), idx_all.cpu()
    assert plan.n_lists == H and ptr[0, 0] == 0 and bool((ptr[:, 1:] >= ptr[:, :-1]).all()) and torch.equal(ptr[1:, 0], ptr[:-1, -1])
    nnz = int(ptr[-1, -1])
    assert nnz <= cap and bool((idx[nnz:] == -7).all()) and bool((ws_all[need:] == 0xA5).all()), "guard words were written"
    lists = [[idx[ptr[h, i]:ptr[h, i + 1]].tolist() for i in range(nt)] for h in range(H)]
    return plan, b, lists


@pytest.mark.parametrize("params", PARAMS, ids=ids)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("geo", GEOS, ids=ids)
def test_lists_follow_the_rule(sel, geo, H, params):
    base, buf, heads, _ = R.pooled(geo[0], geo[1], H)
    _, b, lists = run_select(sel, base, buf, H, *params)
    kept, undecided = b["kept_mass"].cpu().double(), 0
    for h, (p, rho) in enumerate(heads):
        for i in range(base.n_tiles):
            want, decided, _, (lo_c, hi_c) = R.cut(p[i], rho[i], i, *params)
            got = lists[h][i]
            assert got == sorted(set(got)) and all(0 <= j < base.n_tiles for j in got) and lo_c <= len(got) <= hi_c and i in got, (h, i, got)
            m, bound = R.mass_and_bound(p[i], rho[i], got)
            assert abs(float(kept[h, i]) - m) <= bound, (h, i, float(kept[h, i]), m, bound)
            undecided += not decided
            assert not decided or got == want, f"head {h} tile {i}: kernel {got}, rule {want}"
    print(f"select {geo} H={H} {params}: {undecided} of {H * base.n_tiles} rows undecided")
    assert undecided <= 0.05 * H * base.n_tiles


@pytest.mark.parametrize("geo", [GEOS[1], GEOS[3]], ids=ids)
def test_cdf_one_is_the_whole_grid_window(sel, geo):
    from hunyuanvideo_efficiency_amd import ops
    H = 3
    base, buf = R.make_inputs(geo[0], geo[1], H, extra_rows=5)
    plan, _, _ = run_select(sel, base, buf, H, 1.0, 1, None)
    full = ops.tile_plan(geo[0], geo[1], [(99, 99, 99)] * H, DEV)
    nnz = full.nb_idx.numel()
    assert torch.equal(plan.nb_ptr, full.nb_ptr) and torch.equal(plan.nb_idx[:nnz], full.nb_idx)
    gb, n = buf.to(DEV), base.n_img
    q, k, v = gb[:, :H * D], gb[:, H * D:2 * H * D], gb[:, 2 * H * D:3 * H * D]
    outs = [ops.attn_fwd_tile(q[:n], k, v, torch.zeros(n, H * D, dtype=torch.bfloat16, device=DEV), H, pl, dense=(n, n + 5)) for pl in (plan, full)]
    assert torch.equal(outs[0], outs[1])


def test_lists_drive_the_tile_kernel(sel):
    from hunyuanvideo_efficiency_amd import ops
    grid, tile, H, n_dense = (3, 5, 9), (2, 2, 4), 3, 65
    base, buf = R.make_inputs(grid, tile, H, extra_rows=n_dense + 3)
    plan, _, lists = run_select(sel, base, buf, H, 0.9, 2, 5)
    gb, n = buf.to(DEV), base.n_img
    q, k, v = gb[:, :H * D], gb[:, H * D:2 * H * D], gb[:, 2 * H * D:3 * H * D]
    out = ops.attn_fwd_tile(q[:n], k, v, torch.zeros(n, H * D, dtype=torch.bfloat16, device=DEV), H, plan, dense=(n, n + n_dense))
    rows_of = [base.perm[a:b].long() for a, b in zip(base.tile_start[:-1], base.tile_start[1:])]
    worst = 0.0
    for h in range(H):
        cols = slice(h * D, (h + 1) * D)
        for i, rows in enumerate(rows_of):
            keys = torch.cat([rows_of[j] for j in lists[h][i]] + [torch.arange(n, n + n_dense)]).to(DEV)
            ref = AB.AttnRef(q[rows.to(DEV)][:, cols], k[keys][:, cols], v[keys][:, cols], 1, gap=AB.THR)
            worst = max(worst, ref.check_o(out[rows.to(DEV)][:, cols], f"head {h} tile {i} lists {lists[h][i]}"))
    print(f"tile attention under selected lists: worst error / bound {worst:.3f}")


def test_tiny_model_under_the_flag(sel):
    from hunyuanvideo_efficiency_amd.attn_tile import enable_sliding_tile_attention
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.fp8_optimization import enable_fp8_attention
    from tests.test_gpu_attn_tile import _tiny_model_run
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    model = build_model(cfg, DEV)
    off = _tiny_model_run(model, cfg)                           # 5 x 8 x 8 tokens: tiles of (2, 4, 4) make a 3 x 2 x 2 tile grid
    enable_sliding_tile_attention(model, tile=(2, 4, 4), window=(3, 3, 3))
    window = _tiny_model_run(model, cfg)
    with pytest.raises(ValueError):
        sel.enable_adaptive_tile_attention(model, tile=(2, 4, 4))
    enable_sliding_tile_attention(model, enable=False)
    assert sel.enable_adaptive_tile_attention(model, tile=(2, 4, 4), cdf=1.0) == 3
    assert torch.equal(_tiny_model_run(model, cfg), window), "cdf = 1 is not the whole-grid window"
    sel.enable_adaptive_tile_attention(model, tile=(2, 4, 4), cdf=0.5)
    half = _tiny_model_run(model, cfg)
    assert bool(torch.isfinite(half).all()) and not torch.equal(half, window) and not torch.equal(half, off)
    enable_fp8_attention(model)
    with pytest.raises(NotImplementedError, match="tile_plan.*fp8_attention"):
        _tiny_model_run(model, cfg)
    enable_fp8_attention(model, False)
    blocks = list(model.double_blocks) + list(model.single_blocks)
    for block in blocks:
        block.hybrid_seq_parallel_attn = object()
    with pytest.raises(NotImplementedError, match="tile_plan.*hybrid_seq_parallel_attn"):
        _tiny_model_run(model, cfg)
    for block in blocks:
        block.hybrid_seq_parallel_attn = None
    assert sel.enable_adaptive_tile_attention(model, enable=False) == 3 and torch.equal(_tiny_model_run(model, cfg), off)
