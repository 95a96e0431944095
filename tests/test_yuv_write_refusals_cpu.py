"""CPU only: every refusal and limit include/hv_yuv_write.h documents, checked on the host half of its entry point with made-up pointers,
as tests/test_gssim_refusals_cpu.py does for its header (and skipped, like it, where a GPU is present: a missing guard must never launch
on such pointers); the bindings derived from the header; the generated registration source; the Makefile."""
import ctypes as C
import importlib.util
import os
import re

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import yuv_write_contract as T  # noqa: E402

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
    assert set(T.E) == set(decls) == {"hv_clip_to_yuv420"} == {name for _, name, _ in _abi.YUVW_DECLS}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
        assert e.refuse and e.accept and e.limits
    assert _abi.YUVW_MACROS == {"HV_YUVW_CHROMA_TOPLEFT": 0, "HV_YUVW_CHROMA_MEAN": 1}
    # the layouts and the side limit are the main header's, used by value: the new header defines none of its names
    header = open(_abi.YUVW_HEADER).read()
    assert not re.search(r"#define\s+HV_YUV_(I420|YV12|NV12|COEF_BITS|MAX_SIDE)\b", header)
    assert (_abi.MACROS["HV_YUV_I420"], _abi.MACROS["HV_YUV_YV12"], _abi.MACROS["HV_YUV_NV12"], _abi.MACROS["HV_YUV_MAX_SIDE"]) == (0, 1, 2, 16384)
    assert "HV_YUV_I420 = 0" in header and "HV_YUV_YV12 = 1" in header and "HV_YUV_NV12 = 2" in header and "16384" in header
    assert "UNPINNED RESTATEMENT" in header
    # the new header shares no name with the other four, and theirs are what they were
    names = [{n for _, n, _ in d} for d in (_abi.YUVW_DECLS, _abi.GSSIM_DECLS, _abi.TEMPORAL_DECLS, _abi.CONTENT_DECLS, _abi.DECLS)]
    assert not names[0] & (names[1] | names[2] | names[3] | names[4])
    assert not set(_abi.YUVW_MACROS) & (set(_abi.MACROS) | set(_abi.CONTENT_MACROS) | set(_abi.TEMPORAL_MACROS) | set(_abi.GSSIM_MACROS))
    assert _abi.MACROS["HV_ABI_VERSION"] == 11 and "hv_yuv420_to_clip" in names[4] and "hv_gaussian_ssim" in names[1]
    # the ctypes table against the signature typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_clip_to_yuv420": ([p, i, i, l, l, l, i, i, i, i, i, i, p, p], i)}
    assert set(pins) == set(_lib.YUVW_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.YUVW_SIGNATURES[name] == argtypes and _lib.YUVW_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    assert str(hv.clip_to_yuv420.default._schema) == \
        "hv::clip_to_yuv420(Tensor? x, int dtype, int C, int sc, int st, int sh, int T, int H, int W, int rescale, int layout, int chroma, " \
        "Tensor(a!)? raw) -> ()"


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.YUVW_DECLS, "hv_yuv_write.h")
    assert open(g.YUVW_OUT).read() == text, "include/hv_yuv_write.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 1
    # the other four sources are still what the generator writes from their headers
    assert open(g.OUT).read() == g.gen() and open(g.CONTENT_OUT).read() == g.gen(_abi.CONTENT_DECLS, "hv_content.h")
    assert open(g.TEMPORAL_OUT).read() == g.gen(_abi.TEMPORAL_DECLS, "hv_temporal.h")
    assert open(g.GSSIM_OUT).read() == g.gen(_abi.GSSIM_DECLS, "hv_gssim.h")


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_yuv_write_torch_ops.cpp") == 2 and mk.count("../../include/hv_yuv_write.h") == 2
    assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_yuv_write.hip"))
