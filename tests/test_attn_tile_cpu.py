"""CPU only: the contract of include/hv_attn_tile.h without a GPU - the refusals of its entry point through the C ABI (made-up pointers:
skipped where a GPU is present, a missing guard must never launch on them), the bindings and macros, the generated registration source,
the Makefile, the command-line flags, and the tile plan (built on the host, so all of it is checked here)."""
import ctypes as C
import importlib.util
import math
import os

import pytest
import torch

from hunyuanvideo_efficiency_amd import _abi, _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, ARG, LAUNCH = 0x7f0000001000, -1, -2
no_gpu = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: calls with made-up pointers must not reach a device")


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hvat_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _call(**ov):
    a = dict(q=PTR, k=PTR, v=PTR, o=PTR, stride_q=1152, stride_k=1152, stride_v=1152, stride_o=384, n_q=300, n_kv=370, n_heads=3,
             head_dim=128, scale=0.0884, perm=PTR, tile_start=PTR, n_tiles=2, nb_ptr=PTR, nb_idx=PTR, n_lists=1, dense_lo=300,
             dense_hi=370, stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.ATTN_TILE_DECLS if n == "hv_attn_fwd_tile_bf16")
    return _lib.load().hv_attn_fwd_tile_bf16(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("ov", [dict(n_tiles=0), dict(n_tiles=301), dict(n_lists=2), dict(n_lists=0), dict(perm=None), dict(tile_start=None),
                                dict(nb_ptr=None), dict(nb_idx=None), dict(q=None), dict(o=None), dict(dense_lo=371, dense_hi=370),
                                dict(dense_hi=371), dict(dense_lo=-1), dict(head_dim=64), dict(stride_q=1153), dict(stride_k=1156),
                                dict(stride_o=386), dict(stride_o=256), dict(n_heads=0), dict(n_q=-1), dict(n_kv=299),
                                dict(n_tiles=2 ** 30, n_q=2 ** 30, n_kv=2 ** 30 + 70, dense_lo=0, dense_hi=0)],
                         ids=lambda ov: ",".join(f"{k}={v}" for k, v in ov.items()))
def test_refusals(ov):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert _call() == LAUNCH and _call(n_lists=3) == LAUNCH and _call(dense_lo=370) == LAUNCH and _call(**ov) == ARG
    assert _call(n_q=0, dense_lo=0, dense_hi=0) == 0 and _call(n_q=1, n_tiles=1, stride_o=0) == LAUNCH


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    want = [p, p, p, p, l, l, l, l, i, i, i, i, f, p, p, i, p, p, i, i, i, p]
    lib = _lib.load()
    assert list(_lib.ATTN_TILE_SIGNATURES) == ["hv_attn_fwd_tile_bf16"]
    assert lib.hv_attn_fwd_tile_bf16.argtypes == want == _lib.ATTN_TILE_SIGNATURES["hv_attn_fwd_tile_bf16"]
    assert lib.hv_attn_fwd_tile_bf16.restype is i
    assert _abi.ATTN_TILE_MACROS == ops.ATTN_TILE == {"HV_ATTN_TILE_BM": 256, "HV_ATTN_TILE_KVT": 64, "HV_ATTN_TILE_RING": 3}
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.ATTN_TILE_DECLS, "hv_attn_tile.h")
    assert open(g.ATTN_TILE_OUT).read() == text, "include/hv_attn_tile.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 1
    assert open(g.OUT).read() == g.gen() and "hv_attn_fwd_tile_bf16" not in {n for _, n, _ in _abi.DECLS}     # hv_kernels.h is what it was
    schema = str(_lib.torch_ops().attn_fwd_tile_bf16.default._schema)
    assert schema.startswith("hv::attn_fwd_tile_bf16(Tensor? q, Tensor? k, Tensor? v, Tensor(a!)? o, int stride_q,") and \
        schema.endswith("Tensor? perm, Tensor? tile_start, int n_tiles, Tensor? nb_ptr, Tensor? nb_idx, int n_lists, int dense_lo, int dense_hi) -> ()")
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_attn_tile_torch_ops.cpp") == 2 and mk.count("../../include/hv_attn_tile.h") == 2
    assert "../lib/obj/hv_attn_tile.o: FLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops" in mk


def test_sample_video_flags_and_their_pairing(capsys):
    mod = _load_script("sample_video.py")
    a = mod.parse_args([])
    assert a.sliding_tile_attention is False and a.sta_tile is None and a.sta_window is None
    a = mod.parse_args(["--sliding-tile-attention", "--sta-tile", "6", "8", "4", "--sta-window", "3", "3", "5"])
    assert a.sliding_tile_attention is True and a.sta_tile == [6, 8, 4] and a.sta_window == [3, 3, 5]
    for lone in (["--sta-tile", "4", "8", "8"], ["--sta-window", "3", "3", "3"]):
        with pytest.raises(SystemExit):
            mod.parse_args(lone)
        assert "only valid with --sliding-tile-attention" in capsys.readouterr().err


@pytest.mark.parametrize("grid,tile,windows", [((3, 5, 9), (2, 2, 4), [(1, 1, 1)]), ((2, 9, 16), (1, 8, 8), [(3, 3, 3)]),
                                               ((5, 8, 10), (4, 8, 8), [(1, 1, 2), (1, 1, 1), (2, 1, 2)]), ((7, 1, 1), (1, 1, 1), [(4, 9, 2)])])
def test_plan(grid, tile, windows):
    plan = ops.tile_plan(grid, tile, windows[0] if len(windows) == 1 else windows, "cpu")
    nt = [-(-g // t) for g, t in zip(grid, tile)]
    assert (plan.n_img, plan.n_tiles, plan.n_lists) == (math.prod(grid), math.prod(nt), len(windows))
    assert torch.equal(plan.perm.sort().values, torch.arange(plan.n_img, dtype=torch.int32)), "perm is not a permutation"
    counts = plan.tile_start.diff()
    assert plan.tile_start[0] == 0 and plan.tile_start[-1] == plan.n_img and 1 <= int(counts.min()) and int(counts.max()) <= 256
    # a slot's token lies in the slot's tile, and keeps raster order inside it
    t, h, w = plan.perm // (grid[1] * grid[2]), plan.perm // grid[2] % grid[1], plan.perm % grid[2]
    tile_of_slot = ((t // tile[0]) * nt[1] + h // tile[1]) * nt[2] + w // tile[2]
    assert torch.equal(tile_of_slot, torch.repeat_interleave(torch.arange(plan.n_tiles), counts.long()))
    assert all(bool((plan.perm[a:b].diff() > 0).all()) for a, b in zip(plan.tile_start[:-1], plan.tile_start[1:]))
    for l, win in enumerate(windows):                          # the STA rule: every tile attends prod(min(w, tiles)) tiles, each once
        n_nb = math.prod(min(x, n) for x, n in zip(win, nt))
        assert torch.equal(plan.nb_ptr[l].diff(), torch.full((plan.n_tiles,), n_nb, dtype=torch.int32))
        lists = plan.nb_idx[plan.nb_ptr[l, 0]:plan.nb_ptr[l, -1]].view(plan.n_tiles, n_nb)
        assert all(len(set(row.tolist())) == n_nb and i in row.tolist() for i, row in enumerate(lists))
    assert 0.0 < plan.fraction <= 1.0


def test_window_clamp_by_hand_and_tile_limit():
    # 7 tiles along T, window 4 (two tiles before the centre, one behind): 0 -> 0..3, 1 -> 0..3, 2 -> 0..3, 3 -> 1..4, 4 -> 2..5, 5, 6 -> 3..6
    plan = ops.tile_plan((7, 1, 1), (1, 1, 1), (4, 1, 1), "cpu")
    assert plan.nb_idx.view(7, 4).tolist() == [[0, 1, 2, 3]] * 3 + [[1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 6], [3, 4, 5, 6]]
    assert ops.tile_plan((5, 1, 1), (1, 1, 1), (3, 1, 1), "cpu").nb_idx.view(5, 3).tolist() == [[0, 1, 2], [0, 1, 2], [1, 2, 3], [2, 3, 4], [2, 3, 4]]
    assert ops.tile_plan((2, 2, 2), (1, 1, 1), (9, 9, 9), "cpu").fraction == 1.0
    assert abs(ops.tile_plan((5, 1, 1), (1, 1, 1), (3, 1, 1), "cpu").fraction - 15 / 25) < 1e-12
    for bad in (dict(tile=(4, 8, 9)), dict(tile=(1, 1, 257)), dict(window=(0, 1, 1)), dict(window=[(1, 1, 1), (1, 0, 1)])):
        with pytest.raises(ValueError):
            ops.tile_plan(**{**dict(grid=(8, 16, 16), tile=(4, 8, 8), window=(3, 3, 3), device="cpu"), **bad})
