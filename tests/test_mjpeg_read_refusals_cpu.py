"""CPU only: every refusal and limit include/hv_mjpeg_read.h documents, checked on the host half of its entry points with made-up
pointers (the Huffman and quantisation tables are host arrays and real), as tests/test_mjpeg_refusals_cpu.py does for its header (and
skipped, like it, where a GPU is present: a missing guard must never launch on such pointers); the size query; the bindings derived
from the header; the generated registration source; the Makefile."""
import ctypes as C
import importlib.util
import os
import re

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import mjpeg_read_contract as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"hv_mjpeg_find_restarts", "hv_mjpeg_decode_coefs", "hv_mjpeg_coefs_to_clip"}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name,overrides,want", [pytest.param(n, ov, w, id=i) for i, n, ov, w in T.rows()])
def test_row(lib, name, overrides, want):
    """baseline: -2 (accepted, the launch fails without a device); refusal: -1; accept / last value inside a limit: -2"""
    assert T.call(lib, name, overrides) == want


@pytest.mark.parametrize("shape,want", T.QUERY, ids=[str(s) for s, _ in T.QUERY])
def test_size_query(lib, shape, want):
    assert lib.hv_mjpeg_coef_bytes(*shape) == want


def test_the_size_is_exact(lib):
    """the kernels take the query's answer and refuse one byte less, at shapes with one and with several MCUs"""
    for H, W, Ri, ipf in ((16, 32, 1, 2), (17, 33, 0, 1), (1, 1, 0, 1)):
        need = lib.hv_mjpeg_coef_bytes(1, H, W)
        strides = dict(sh=W, sc=H * W, st=3 * H * W)
        assert T.call(lib, "hv_mjpeg_decode_coefs", dict(H=H, W=W, Ri=Ri, ipf=ipf, coef_bytes=need)) == T.LAUNCH
        assert T.call(lib, "hv_mjpeg_decode_coefs", dict(H=H, W=W, Ri=Ri, ipf=ipf, coef_bytes=need - 1)) == T.ARG
        assert T.call(lib, "hv_mjpeg_coefs_to_clip", dict(H=H, W=W, coef_bytes=need, **strides)) == T.LAUNCH
        assert T.call(lib, "hv_mjpeg_coefs_to_clip", dict(H=H, W=W, coef_bytes=need - 1, **strides)) == T.ARG


def test_the_table_covers_the_header_and_the_header_is_bound():
    decls = T.stream_decls()
    assert set(T.E) == set(decls) == NAMES
    assert {name for _, name, _ in _abi.MJPEG_READ_DECLS} == NAMES | {"hv_mjpeg_coef_bytes"}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
        assert e.refuse and e.accept and e.limits
    assert _abi.MJPEG_READ_MACROS == {"HV_MJPEG_HUFF_BYTES": 1088, "HV_MJPEG_QUANT_BYTES": 128, "HV_MJPEG_COEF_BYTES_PER_MCU": 768,
                                      "HV_MJPEG_RST_ORDER": 1 << 30}
    # the side limit is the main header's, used by value; that header, hv_mjpeg.h and the ABI version are what they were
    header = open(_abi.MJPEG_READ_HEADER).read()
    assert not re.search(r"#define\s+HV_YUV_\w+", header) and "16384" in header
    assert _abi.MACROS["HV_YUV_MAX_SIDE"] == 16384 and _abi.MACROS["HV_ABI_VERSION"] == 11
    assert {n for _, n, _ in _abi.MJPEG_DECLS} == {"hv_mjpeg_measure", "hv_mjpeg_write"}
    others = (_abi.MJPEG_DECLS, _abi.MOTION_DECLS, _abi.YUVW_DECLS, _abi.GSSIM_DECLS, _abi.TEMPORAL_DECLS, _abi.CONTENT_DECLS, _abi.DECLS)
    mine = {n for _, n, _ in _abi.MJPEG_READ_DECLS}
    assert not any(mine & {n for _, n, _ in d} for d in others)
    assert not set(_abi.MJPEG_READ_MACROS) & (set(_abi.MACROS) | set(_abi.CONTENT_MACROS) | set(_abi.TEMPORAL_MACROS) | set(_abi.GSSIM_MACROS) |
                                              set(_abi.YUVW_MACROS) | set(_abi.MOTION_MACROS) | set(_abi.MJPEG_MACROS))
    # the ctypes table against the signatures typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_mjpeg_coef_bytes": ([i, i, i], l),
            "hv_mjpeg_find_restarts": ([p, l, p, p, i, i, p, p, p, p], i),
            "hv_mjpeg_decode_coefs": ([p, l, p, p, i, i, i, i, i, p, p, l, p, p], i),
            "hv_mjpeg_coefs_to_clip": ([p, l, p, p, p, i, l, l, l, i, i, i, p], i)}
    assert set(pins) == set(_lib.MJPEG_READ_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.MJPEG_READ_SIGNATURES[name] == argtypes and _lib.MJPEG_READ_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    assert str(hv.mjpeg_coef_bytes.default._schema) == "hv::mjpeg_coef_bytes(int T, int H, int W) -> int"
    assert str(hv.mjpeg_find_restarts.default._schema) == (
        "hv::mjpeg_find_restarts(Tensor? data, int data_bytes, Tensor? scan_begin, Tensor? scan_end, int T, int ipf, "
        "Tensor(a!)? interval_begin, Tensor(b!)? interval_end, Tensor(c!)? found) -> ()")
    assert str(hv.mjpeg_decode_coefs.default._schema) == (
        "hv::mjpeg_decode_coefs(Tensor? data, int data_bytes, Tensor? interval_begin, Tensor? interval_end, int T, int H, int W, int Ri, "
        "int ipf, int[] huff_tables, Tensor(a!)? coefs, int coef_bytes, Tensor(b!)? status) -> ()")
    assert str(hv.mjpeg_coefs_to_clip.default._schema) == (
        "hv::mjpeg_coefs_to_clip(Tensor? coefs, int coef_bytes, int[] quant_tables, Tensor? vtab, Tensor(a!)? out, int dtype, int sc, "
        "int st, int sh, int T, int H, int W) -> ()")
    assert int(hv.mjpeg_coef_bytes(2, 17, 33)) == 2 * 6 * 768


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.MJPEG_READ_DECLS, "hv_mjpeg_read.h")
    assert open(g.MJPEG_READ_OUT).read() == text, "include/hv_mjpeg_read.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 4
    assert "huff_tables.size() == 1088" in text and "quant_tables.size() == 128" in text
    # the other sources are still what the generator writes from their headers
    assert open(g.OUT).read() == g.gen() and open(g.MJPEG_OUT).read() == g.gen(_abi.MJPEG_DECLS, "hv_mjpeg.h")
    assert open(g.YUVW_OUT).read() == g.gen(_abi.YUVW_DECLS, "hv_yuv_write.h")


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_mjpeg_read_torch_ops.cpp") == 2 and mk.count("../../include/hv_mjpeg_read.h") == 2
    assert "hv_mjpeg_decode.hpp" in mk
    for name in ("hv_mjpeg_read.hip", "hv_mjpeg_decode.hpp"):
        assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", name))


def test_the_sources_carry_the_constants_of_the_restatement():
    """the zigzag table of csrc/hv_mjpeg_decode.hpp and the constants of the inverse DCT and the colour rule in csrc/hv_mjpeg_read.hip against
    tests/mjpeg_ref.py (which derives the zigzag from its definition) and the header"""
    from tests import mjpeg_ref as R
    hpp = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_decode.hpp")).read()
    body = re.search(r"nat\[64\]\s*=\s*\{(.*?)\};", hpp, flags=re.S).group(1)
    assert [int(v) for v in re.findall(r"\d+", body)] == R.ZIG
    hip = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_read.hip")).read()
    header = open(_abi.MJPEG_READ_HEADER).read()
    for c in (2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172, 91881, 22554, 46802, 116130):
        assert str(c) in hip and str(c) in header, c
