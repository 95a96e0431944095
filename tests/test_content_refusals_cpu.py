"""CPU only: every refusal, limit and early-out include/hv_content.h documents, checked on the host half of its entry points with made-up
pointers, as tests/test_capi_refusals_cpu.py does for include/hv_kernels.h (and skipped, like it, where a GPU is present: a missing guard
must never launch on such pointers); the bindings derived from the header; the generated registration source."""
import ctypes as C
import importlib.util
import os

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import content_contract as T  # noqa: E402
from tests.abi_contract import sweep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name,overrides,want", [pytest.param(n, ov, w, id=i) for i, n, ov, w in T.rows()])
def test_row(lib, name, overrides, want):
    """baseline: -2 (accepted, the launch fails without a device); refusal: -1; accept / last value inside a limit: -2; early-out: 0"""
    assert T.call(lib, name, overrides) == want


def test_the_table_covers_the_header_and_the_header_is_bound():
    decls = T.stream_decls()
    assert set(T.E) == set(decls) == {"hv_content_histograms", "hv_histogram_entropy"}
    assert set(T.QUERIES) == {name for _, name, params in _abi.CONTENT_DECLS if name not in decls and params}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
    used = {m for e in T.E.values() for _, macros, _, _ in e.limits for m in macros}
    assert used == set(_abi.CONTENT_MACROS) == {"HV_CONTENT_CHUNK", "HV_CONTENT_INTER_BINS"}
    assert _abi.CONTENT_MACROS == {"HV_CONTENT_CHUNK": 8192, "HV_CONTENT_INTER_BINS": 511}
    # nothing of this header leaks into the main one: its declarations, constants and version are the recorded ABI's
    assert not {n for _, n, _ in _abi.CONTENT_DECLS} & {n for _, n, _ in _abi.DECLS} and not set(_abi.CONTENT_MACROS) & set(_abi.MACROS)
    # the ctypes table against signatures typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_content_histograms": ([p, l, l, l, i, i, i, i, i, i, i, i, i, i, p, p, p, l, p], i),
            "hv_content_histograms_workspace_bytes": ([i, i, i], l), "hv_histogram_entropy": ([p, l, i, i, p, p], i)}
    assert set(pins) == set(_lib.CONTENT_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.CONTENT_SIGNATURES[name] == argtypes and _lib.CONTENT_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    for name in pins:
        assert getattr(hv, name[len("hv_"):]).default._schema.name == "hv::" + name[len("hv_"):]


@pytest.mark.parametrize("name", sorted(T.QUERIES))
def test_host_query(lib, name):
    """0 for the shapes its kernel refuses, the documented value elsewhere, and never a negative number"""
    fn = getattr(lib, name)
    for args, want in T.QUERIES[name]:
        got = fn(*args)
        assert (got > 0) if want is None else (got == want), (name, args, got, want)
    for args in sweep(len(_lib.CONTENT_SIGNATURES[name])):
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
    text = g.gen(_abi.CONTENT_DECLS, "hv_content.h")
    assert open(g.CONTENT_OUT).read() == text, "include/hv_content.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 3
