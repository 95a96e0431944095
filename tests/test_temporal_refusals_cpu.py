"""CPU only: every refusal and limit include/hv_temporal.h documents, checked on the host half of its entry point with made-up pointers,
as tests/test_content_refusals_cpu.py does for include/hv_content.h (and skipped, like it, where a GPU is present: a missing guard must
never launch on such pointers); the bindings derived from the header; the generated registration source."""
import ctypes as C
import importlib.util
import os

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import temporal_contract as T  # noqa: E402

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
    assert set(T.E) == set(decls) == {n for _, n, _ in _abi.TEMPORAL_DECLS} == {"hv_temporal_interp_f16"}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
        assert e.refuse and e.accept and e.limits
    assert _abi.TEMPORAL_MACROS == {}
    # the new header shares no name with the other two, and theirs are what they were: the recorded ABI and the content entry points
    names = [{n for _, n, _ in d} for d in (_abi.TEMPORAL_DECLS, _abi.CONTENT_DECLS, _abi.DECLS)]
    assert not names[0] & names[1] and not names[0] & names[2] and not names[1] & names[2]
    assert not set(_abi.TEMPORAL_MACROS) & (set(_abi.MACROS) | set(_abi.CONTENT_MACROS))
    assert _abi.MACROS["HV_ABI_VERSION"] == 11 and "hv_temporal_resample_f16" in names[2]
    # the ctypes table against the signature typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_temporal_interp_f16": ([p, l, p, l, i, l, i, i, p], i)}
    assert set(pins) == set(_lib.TEMPORAL_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.TEMPORAL_SIGNATURES[name] == argtypes and _lib.TEMPORAL_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    for name in pins:
        assert getattr(hv, name[len("hv_"):]).default._schema.name == "hv::" + name[len("hv_"):]
    assert str(hv.temporal_interp_f16.default._schema) == \
        "hv::temporal_interp_f16(Tensor? x, int ldx, Tensor(a!)? out, int ldo, int T_in, int HW, int C, int s) -> ()"


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.TEMPORAL_DECLS, "hv_temporal.h")
    assert open(g.TEMPORAL_OUT).read() == text, "include/hv_temporal.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 1
    # the other two sources are still what the generator writes from their headers
    assert open(g.OUT).read() == g.gen() and open(g.CONTENT_OUT).read() == g.gen(_abi.CONTENT_DECLS, "hv_content.h")


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_temporal_torch_ops.cpp") == 2 and "../../include/hv_temporal.h" in mk
    assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_temporal.hip"))
