"""CPU only: every refusal and limit include/hv_gssim.h documents, checked on the host half of its entry point with made-up pointers, as
tests/test_content_refusals_cpu.py and tests/test_temporal_refusals_cpu.py do for their headers (and skipped, like them, where a GPU is
present: a missing guard must never launch on such pointers); the bindings derived from the header; the generated registration source;
the Makefile."""
import ctypes as C
import importlib.util
import os

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import gssim_contract as T  # noqa: E402
from tests.abi_contract import sweep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name,overrides,want", [pytest.param(n, ov, w, id=i) for i, n, ov, w in T.rows()])
def test_row(lib, name, overrides, want):
    """baseline: -2 (accepted, the launch fails without a device); refusal: -1; accept / last value inside a limit: -2"""
    assert T.call(lib, name, overrides) == want


def test_the_table_covers_the_header_and_the_header_is_bound():
    decls = T.stream_decls()
    assert set(T.E) == set(decls) == {"hv_gaussian_ssim"}
    assert set(T.QUERIES) == {name for _, name, params in _abi.GSSIM_DECLS if name not in decls and params}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
        assert e.refuse and e.accept and e.limits
    used = {m for e in T.E.values() for _, macros, _, _ in e.limits for m in macros}
    assert used == set(_abi.GSSIM_MACROS) == {"HV_GSSIM_WIN", "HV_GSSIM_TILE_H", "HV_GSSIM_TILE_W"}
    assert _abi.GSSIM_MACROS == {"HV_GSSIM_WIN": 11, "HV_GSSIM_TILE_H": 16, "HV_GSSIM_TILE_W": 32}
    # the new header shares no name with the other three, and theirs are what they were
    names = [{n for _, n, _ in d} for d in (_abi.GSSIM_DECLS, _abi.TEMPORAL_DECLS, _abi.CONTENT_DECLS, _abi.DECLS)]
    assert not names[0] & (names[1] | names[2] | names[3])
    assert not set(_abi.GSSIM_MACROS) & (set(_abi.MACROS) | set(_abi.CONTENT_MACROS) | set(_abi.TEMPORAL_MACROS))
    assert _abi.MACROS["HV_ABI_VERSION"] == 11 and "hv_video_metrics" in names[3]
    # the ctypes table against the signatures typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_gaussian_ssim": ([p, l, l, l, p, l, l, l, i, i, i, i, i, i, i, p, p, p, l, p], i),
            "hv_gaussian_ssim_workspace_bytes": ([i, i, i, i, i], l)}
    assert set(pins) == set(_lib.GSSIM_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.GSSIM_SIGNATURES[name] == argtypes and _lib.GSSIM_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    assert str(hv.gaussian_ssim.default._schema) == \
        "hv::gaussian_ssim(Tensor? a, int a_sc, int a_st, int a_sh, Tensor? b, int b_sc, int b_st, int b_sh, int dtype, int C, int T, " \
        "int H, int W, int rescale, int temporal, Tensor? win, Tensor(a!)? ssim_sum, Tensor(b!)? workspace, int workspace_bytes) -> ()"
    assert str(hv.gaussian_ssim_workspace_bytes.default._schema) == \
        "hv::gaussian_ssim_workspace_bytes(int C, int T, int H, int W, int temporal) -> int"


@pytest.mark.parametrize("name", sorted(T.QUERIES))
def test_host_query(lib, name):
    """0 for the shapes its kernel refuses, the documented value elsewhere, and never a negative number"""
    fn = getattr(lib, name)
    for args, want in T.QUERIES[name]:
        got = fn(*args)
        assert (got > 0) if want is None else (got == want), (name, args, got, want)
    for args in sweep(len(_lib.GSSIM_SIGNATURES[name])):
        assert fn(*args) >= 0, (name, args)


@pytest.mark.parametrize("query,qargs,kernel,param,scale", T.SIZE_RULES, ids=[r[0] for r in T.SIZE_RULES])
def test_size_query_is_the_kernels_own_minimum(lib, query, qargs, kernel, param, scale):
    size = getattr(lib, query)(*qargs) * scale
    assert size > 0
    assert T.call(lib, kernel, {param: size}) == T.LAUNCH
    assert T.call(lib, kernel, {param: size - 1}) == T.ARG


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.GSSIM_DECLS, "hv_gssim.h")
    assert open(g.GSSIM_OUT).read() == text, "include/hv_gssim.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 2
    # the other three sources are still what the generator writes from their headers
    assert open(g.OUT).read() == g.gen() and open(g.CONTENT_OUT).read() == g.gen(_abi.CONTENT_DECLS, "hv_content.h")
    assert open(g.TEMPORAL_OUT).read() == g.gen(_abi.TEMPORAL_DECLS, "hv_temporal.h")


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_gssim_torch_ops.cpp") == 2 and mk.count("../../include/hv_gssim.h") == 2
    assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_gssim.hip"))
