"""CPU only: include/hv_attn_select.h without a GPU - the bindings, macros, generated registration source and Makefile; every refusal of
the header through the C ABI (made-up pointers: skipped where a GPU is present, a missing guard must never launch on them); the float64
restatement (tests/attn_select_ref.py) on hand-made rows; the undecided-share condition of tests/test_gpu_attn_select.py on its inputs;
the command-line flags; and that no new wrapper is public in ops."""
import ctypes as C
import os

import numpy as np
import pytest

from hunyuanvideo_efficiency_amd import _abi, _lib, attn_select, ops
from tests import attn_select_ref as R
from tests.test_attn_tile_cpu import ARG, LAUNCH, PTR, ROOT, _load_script, no_gpu
from tests.test_gpu_attn_select import GEOS, PARAMS, ids


def _call(**ov):
    a = dict(q=PTR, k=PTR, stride_q=1152, stride_k=1152, n_q=300, n_heads=3, head_dim=128, scale=0.0884, perm=PTR, tile_start=PTR,
             n_tiles=40, cdf=0.9, k_min=2, k_max=5, nb_ptr=PTR, nb_idx=PTR, nb_idx_capacity=600, kept_mass=None, workspace=PTR,
             workspace_bytes=_lib.load().hv_attn_select_workspace_bytes(40, 3), stream=None)
    a.update(ov)
    params = next(p for _, n, p in _abi.ATTN_SELECT_DECLS if n == "hv_attn_select_tiles")
    return _lib.load().hv_attn_select_tiles(*[a[p] for _, p in params])


@no_gpu
@pytest.mark.parametrize("ov", [dict(q=None), dict(k=None), dict(perm=None), dict(tile_start=None), dict(nb_ptr=None), dict(nb_idx=None),
                                dict(workspace=None), dict(q=PTR + 8), dict(workspace=PTR + 4), dict(head_dim=64), dict(n_heads=0),
                                dict(n_heads=65536), dict(n_tiles=0), dict(n_tiles=1025, n_q=2000), dict(n_tiles=301), dict(stride_q=1156),
                                dict(stride_k=1153), dict(cdf=0.0), dict(cdf=1.0001), dict(cdf=float("nan")), dict(k_min=0), dict(k_min=6),
                                dict(nb_idx_capacity=599), dict(k_max=41, nb_idx_capacity=4799), dict(workspace_bytes=1000)],
                         ids=lambda ov: ",".join(f"{k}={v}" for k, v in ov.items()))
def test_refusals(ov):
    """the accepted call fails at the launch (-2: no device), each refusal before it (-1)"""
    assert _call() == LAUNCH and _call(cdf=1.0, kept_mass=PTR) == LAUNCH and _call(k_max=41, nb_idx_capacity=4800) == LAUNCH
    assert _call(**ov) == ARG


def test_the_header_is_bound_and_the_generated_source_is_up_to_date():
    p, i, l, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    lib = _lib.load()
    want = {"hv_attn_select_workspace_bytes": [i, i], "hv_attn_select_tiles": [p, p, l, l, i, i, i, f, p, p, i, f, i, i, p, p, l, p, p, l, p]}
    assert _lib.ATTN_SELECT_SIGNATURES == want and all(getattr(lib, n).argtypes == a for n, a in want.items())
    assert lib.hv_attn_select_workspace_bytes.restype is l and lib.hv_attn_select_tiles.restype is i
    assert _abi.ATTN_SELECT_MACROS == attn_select.ATTN_SELECT == {"HV_ATTN_SELECT_MAX_TILES": 1024, "HV_ATTN_SELECT_BAND": 32}
    words = lambda nt: 2 * ((nt + 63) // 64)
    assert [lib.hv_attn_select_workspace_bytes(nt, h) for nt, h in ((0, 3), (1025, 3), (40, 0))] == [0, 0, 0]
    assert lib.hv_attn_select_workspace_bytes(1020, 24) == 24 * 1020 * (2 * 512 + 4 + 4 * words(1020))     # the 720p x 257-frame grid
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.ATTN_SELECT_DECLS, "hv_attn_select.h")
    assert open(g.ATTN_SELECT_OUT).read() == text, "include/hv_attn_select.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 2
    assert open(g.OUT).read() == g.gen() and not {n for _, n, _ in _abi.DECLS} & set(want)                # hv_kernels.h is what it was
    assert str(_lib.torch_ops().attn_select_tiles.default._schema).endswith(
        "int k_max, Tensor(a!)? nb_ptr, Tensor(b!)? nb_idx, int nb_idx_capacity, Tensor(c!)? kept_mass, Tensor(d!)? workspace, int workspace_bytes) -> ()")
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert mk.count("hv_attn_select_torch_ops.cpp") == 2 and mk.count("../../include/hv_attn_select.h") == 2


def test_the_restatement_on_hand_made_rows():
    z = np.zeros(4)
    cut = lambda p, i, *a: R.cut(np.array(p), z[:len(p)], i, *a)[:2]
    assert cut([0.1, 0.3, 0.3, 0.3], 0, 0.6, 1, None) == ([0, 1, 2], False)        # a tie at the cut: by tile index, and not decided
    assert cut([0.1, 0.3, 0.3, 0.3], 0, 0.75, 1, None) == ([0, 1, 2, 3], True)     # the tie inside the prefix decides nothing
    assert cut([0.5, 0.45, 0.05], 2, 0.5, 1, None) == ([0, 2], True)                # the own tile ranks first though its p is last
    assert cut([0.5, 0.45, 0.05], 2, 0.04, 1, None) == ([2], True)
    assert cut([0.2, 0.7, 0.1], 0, 0.5, 7, 9) == ([0, 1, 2], True)                  # k_min > n_tiles: every tile
    assert cut([0.2, 0.7, 0.1], 0, 1.0, 1, 2) == ([0, 1], True)                     # cdf = 1 with a small k_max: top-k
    assert cut([0.5, 0.25, 0.25], 0, 0.5, 1, None) == ([0], False)                  # cdf reached exactly: fp32 may fall either side
    assert cut([0.5, 0.25, 0.25], 0, 0.5, 1, 1) == ([0], True)                      # ... unless the clamp takes the question away


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("geo", GEOS, ids=ids)
def test_the_test_inputs_leave_few_rows_undecided(geo, H):
    base, _, heads, _ = R.pooled(geo[0], geo[1], H)
    for params in PARAMS:
        undecided = sum(not R.cut(p[i], rho[i], i, *params)[1] for p, rho in heads for i in range(base.n_tiles))
        assert undecided <= 0.05 * H * base.n_tiles, (params, undecided)
    spread = np.mean([np.log2(p.max(1) / p.min(1)).mean() for p, _ in heads])
    assert base.n_tiles == 1 or spread > 3.0, f"the pooled scores of a row spread over {spread:.2f} units only"


def test_flags_their_pairing_and_the_names(capsys):
    mod = _load_script("sample_video.py")
    a = mod.parse_args([])
    assert a.adaptive_tile_attention is False and (a.ata_tile, a.ata_cdf, a.ata_kmin, a.ata_kmax) == (None,) * 4
    a = mod.parse_args(["--adaptive-tile-attention", "--ata-tile", "2", "8", "8", "--ata-cdf", "0.8", "--ata-kmin", "2", "--ata-kmax", "27"])
    assert a.adaptive_tile_attention is True and (a.ata_tile, a.ata_cdf, a.ata_kmin, a.ata_kmax) == ([2, 8, 8], 0.8, 2, 27)
    for bad, msg in [(["--ata-tile", "4", "8", "8"], "only valid with"), (["--ata-cdf", "0.5"], "only valid with"), (["--ata-kmin", "2"], "only valid with"),
                     (["--ata-kmax", "9"], "only valid with"), (["--adaptive-tile-attention", "--sliding-tile-attention"], "exclude each other")]:
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
        assert msg in capsys.readouterr().err
    for name in ("select_plan", "select_buffers", "plan_density", "enable_adaptive_tile_attention", "ATTN_SELECT"):
        assert hasattr(attn_select, name) and not hasattr(ops, name)
