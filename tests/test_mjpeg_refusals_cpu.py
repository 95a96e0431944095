"""CPU only: every refusal and limit include/hv_mjpeg.h documents, checked on the host half of its entry points with made-up pointers, as
tests/test_yuv_write_refusals_cpu.py does for its header (and skipped, like it, where a GPU is present: a missing guard must never launch
on such pointers); the bindings derived from the header; the generated registration source; the Makefile."""
import ctypes as C
import importlib.util
import os
import re

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import mjpeg_contract as T  # noqa: E402

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
    assert set(T.E) == set(decls) == {"hv_mjpeg_measure", "hv_mjpeg_write"} == {name for _, name, _ in _abi.MJPEG_DECLS}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
        assert e.refuse and e.accept and e.limits
    assert _abi.MJPEG_MACROS == {"HV_MJPEG_DEFAULT_QUALITY": 90, "HV_MJPEG_MCU": 16}
    # the side limit is the main header's, used by value: the new header defines none of its names, and that header is what it was
    header = open(_abi.MJPEG_HEADER).read()
    assert not re.search(r"#define\s+HV_YUV_\w+", header) and "16384" in header
    assert _abi.MACROS["HV_YUV_MAX_SIDE"] == 16384 and _abi.MACROS["HV_ABI_VERSION"] == 11
    others = (_abi.MOTION_DECLS, _abi.YUVW_DECLS, _abi.GSSIM_DECLS, _abi.TEMPORAL_DECLS, _abi.CONTENT_DECLS, _abi.DECLS)
    mine = {n for _, n, _ in _abi.MJPEG_DECLS}
    assert not any(mine & {n for _, n, _ in d} for d in others)
    assert not set(_abi.MJPEG_MACROS) & (set(_abi.MACROS) | set(_abi.CONTENT_MACROS) | set(_abi.TEMPORAL_MACROS) | set(_abi.GSSIM_MACROS) |
                                         set(_abi.YUVW_MACROS) | set(_abi.MOTION_MACROS))
    # the ctypes table against the signatures typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    clip = [p, i, i, l, l, l, i, i, i, i, i]
    pins = {"hv_mjpeg_measure": (clip + [p, p], i), "hv_mjpeg_write": (clip + [p, p, p], i)}
    assert set(pins) == set(_lib.MJPEG_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.MJPEG_SIGNATURES[name] == argtypes and _lib.MJPEG_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    clip = "Tensor? x, int dtype, int C, int sc, int st, int sh, int T, int H, int W, int rescale, int quality, "
    assert str(hv.mjpeg_measure.default._schema) == "hv::mjpeg_measure(" + clip + "Tensor(a!)? interval_bytes) -> ()"
    assert str(hv.mjpeg_write.default._schema) == "hv::mjpeg_write(" + clip + "Tensor? offsets, Tensor(a!)? scan) -> ()"


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.MJPEG_DECLS, "hv_mjpeg.h")
    assert open(g.MJPEG_OUT).read() == text, "include/hv_mjpeg.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 2
    # the other sources are still what the generator writes from their headers
    assert open(g.OUT).read() == g.gen() and open(g.YUVW_OUT).read() == g.gen(_abi.YUVW_DECLS, "hv_yuv_write.h")
    assert open(g.MOTION_OUT).read() == g.gen(_abi.MOTION_DECLS, "hv_motion.h")


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_mjpeg_torch_ops.cpp") == 2 and mk.count("../../include/hv_mjpeg.h") == 2
    assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg.hip"))


def test_the_kernel_source_carries_the_tables_of_the_restatement():
    """the literal tables of csrc/hv_mjpeg.hip (Annex K quantisation, BITS, HUFFVAL, the zigzag, the DCT matrix) against tests/mjpeg_ref.py,
    which derives the zigzag and the matrix from their definitions"""
    from tests import mjpeg_ref as R
    src = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg.hip")).read()

    def table(name):
        body = re.search(re.escape(name) + r"(?:\[\d+\])+\s*=\s*(\{.*?\});", src, flags=re.S).group(1)
        return [int(v, 0) for v in re.findall(r"-?(?:0x[0-9A-Fa-f]+|\d+)", body)]
    assert table("kBaseQ") == R.K1 + R.K2
    assert table("kM") == R.M.reshape(-1).tolist()
    assert table("kHuffBits") == R.DC_L[0] + R.AC_L[0] + R.DC_C[0] + R.AC_C[0]
    assert table("kAcVals") == R.AC_L[1] + R.AC_C[1]
    zig_of = table("kZigOf")
    assert [zig_of[n] for n in R.ZIG] == list(range(64))
