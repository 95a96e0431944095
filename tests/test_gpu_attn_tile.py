"""GPU: the opt-in sliding-tile attention of include/hv_attn_tile.h.

(1) The kernel element by element against fp64 masked attention.  The mask is restated here from (grid, tile, window) with index arithmetic
of its own (`allowed`, tests/attn_tile_plans.py), not read from the plan tensors the kernel consumes: a query may see the image tokens whose tile lies in the clamped
window of its own tile, and the dense range.  Per query tile and head the allowed keys are gathered and handed to AB.AttnRef with
gap = AB.THR (the kernel's running maximum is never deferred: within the contract's threshold); the bound is that of the dense kernel,
tests/attention_bounds.py, unchanged.  `peaked` puts dominant keys inside some tiles' windows and outside others' (and one behind the dense
range): a key outside the window that would own the row must leave no trace.  `phantom` pins the tail mask of every partial chunk.

(2) The tiny model under enable_sliding_tile_attention: a window over the whole grid within 3e-2 of the flagless output's range (the
project's figure for a GPU block against its reference), a one-tile window different and finite, the flag with an SP object or with
fp8_attention an error."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import attention_bounds as AB  # noqa: E402
from tests.attn_tile_plans import allowed  # noqa: E402

DEV = "cuda"
D = 128
GEOS = [((3, 5, 9), (2, 2, 4), (1, 1, 1)),          # ragged in all three axes: tiles of 16, 8, 4, 2 and 1 tokens, a window of one tile
        ((2, 9, 16), (1, 8, 8), (3, 3, 3)),         # a tile of one 64-key chunk, a tile of 8; the window clamps at every border
        ((5, 8, 10), (4, 8, 8), (1, 1, 2)),         # a 256-token tile, ragged tiles of 64, 128 and 32
        ((1, 13, 20), (1, 13, 19), (1, 1, 1)),      # 247 tokens (last chunk 55 keys, last wave partly empty) beside 13 (three waves empty)
        ((3, 5, 9), (2, 2, 4), (9, 9, 9))]          # the window covers the tile grid: full attention in permuted key order


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.torch_ops()
    return _ops


def check_case(ops, grid, tile, windows, n_dense, H, cls):
    n_img = math.prod(grid)
    S = n_img + n_dense + 3                                    # three rows behind the dense range: never a key
    q, k, v = AB.make_case(cls, S, S, H, f"tile.{grid}.{tile}.{n_dense}.{H}", device=DEV)
    buf = torch.cat([q, k, v], 1)                              # q, k, v as views into one fused buffer
    qv, kv, vv = buf[:, :H * D], buf[:, H * D:2 * H * D], buf[:, 2 * H * D:]
    out = torch.full((S, H * D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    plan = ops.tile_plan(grid, tile, windows[0] if len(windows) == 1 else windows, DEV)
    ops.attn_fwd_tile(qv[:n_img], kv, vv, out[:n_img, :H * D], H, plan, dense=(n_img, n_img + n_dense))
    assert bool((out[n_img:] == 7.0).all()) and bool((out[:, H * D:] == 7.0).all()), "rows or columns outside the image output were written"
    worst = 0.0
    for h in range(H):
        ok, tid = allowed(grid, tile, windows[h % len(windows)])
        cols = slice(h * D, (h + 1) * D)
        for t in tid.unique().tolist():
            rows = (tid == t).nonzero()[:, 0]
            keys = torch.cat([ok[rows[0]].nonzero()[:, 0], torch.arange(n_img, n_img + n_dense)]).to(DEV)
            rows = rows.to(DEV)
            ref = AB.AttnRef(qv[rows][:, cols], kv[keys][:, cols], vv[keys][:, cols], 1, gap=AB.THR)
            worst = max(worst, ref.check_o(out[rows][:, cols], f"{cls} {grid}/{tile}/{windows} dense {n_dense} head {h}/{H} tile {t}"))
    print(f"tile attention {cls} {grid}/{tile}/{windows} dense {n_dense} x {H}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("cls", ["random", "peaked", "phantom"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n_dense", [0, 1, 64, 65])
@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "-".join("x".join(map(str, x)) for x in g))
def test_kernel_within_fp64_bound(ops, geo, n_dense, H, cls):
    check_case(ops, geo[0], geo[1], [geo[2]], n_dense, H, cls)


@pytest.mark.parametrize("cls", ["random", "peaked", "phantom"])
def test_one_window_per_head(ops, cls):
    check_case(ops, (5, 8, 10), (4, 8, 8), [(1, 1, 2), (1, 1, 1), (2, 1, 2)], 65, 3, cls)


def _tiny_model_run(model, cfg):
    from hunyuanvideo_efficiency_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    thw, txt_len, n_valid = (5, 16, 16), 32, 11
    x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, thw, txt_len, n_valid, seed=2)
    cos, sin = get_nd_rotary_pos_embed(cfg.rope_dim_list, [thw[0], thw[1] // 2, thw[2] // 2], theta=256, use_real=True)
    with torch.no_grad():
        return model(x.to(DEV), torch.tensor([997.093]).to(DEV), text_states=ts.to(torch.bfloat16).to(DEV), text_mask=tm.to(DEV),
                     text_states_2=ts2.to(DEV), freqs_cos=cos.to(DEV), freqs_sin=sin.to(DEV),
                     guidance=torch.tensor([6016.0]).to(DEV))["x"].float().cpu()


def test_model_with_sliding_tile_attention(ops):
    from hunyuanvideo_efficiency_amd.attn_tile import enable_sliding_tile_attention
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.fp8_optimization import enable_fp8_attention
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    model = build_model(cfg, DEV)
    off = _tiny_model_run(model, cfg)                           # 5 x 8 x 8 tokens: tiles of (2, 4, 4) make a 3 x 2 x 2 tile grid
    assert enable_sliding_tile_attention(model, tile=(2, 4, 4), window=(3, 3, 3)) == 3
    full = _tiny_model_run(model, cfg)
    rel = float((full - off).abs().max() / off.abs().max())
    print(f"sliding-tile attention, tiny model, window over the grid: {rel:.4g} of the output range")
    assert rel < 3e-2, rel
    enable_sliding_tile_attention(model, tile=(2, 4, 4), window=(1, 1, 1))
    one = _tiny_model_run(model, cfg)
    assert bool(torch.isfinite(one).all()) and not torch.equal(one, off), "the sliding-tile path did not run"
    assert enable_sliding_tile_attention(model, enable=False) == 3 and torch.equal(_tiny_model_run(model, cfg), off)
    enable_sliding_tile_attention(model, tile=(2, 4, 4))
    enable_fp8_attention(model)
    with pytest.raises(NotImplementedError, match="tile_plan.*fp8_attention"):
        _tiny_model_run(model, cfg)
    enable_fp8_attention(model, False)
    for block in list(model.double_blocks) + list(model.single_blocks):
        block.hybrid_seq_parallel_attn = object()
    with pytest.raises(NotImplementedError, match="tile_plan.*hybrid_seq_parallel_attn"):
        _tiny_model_run(model, cfg)
