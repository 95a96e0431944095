"""CPU only: every refusal, limit and early-out include/hv_motion.h documents, checked on the host half of its entry point with made-up
pointers, as tests/test_content_refusals_cpu.py does for include/hv_content.h (and skipped, like it, where a GPU is present: a missing
guard must never launch on such pointers); the bindings derived from the header; the generated registration source."""
import ctypes as C
import importlib.util
import os

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import motion_contract as T  # noqa: E402

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
    assert set(T.E) == set(decls) == {"hv_block_motion"} == {n for _, n, _ in _abi.MOTION_DECLS}
    for name, params in decls.items():
        e = T.E[name]
        assert set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*")), name
    used = {m for e in T.E.values() for _, macros, _, _ in e.limits for m in macros}
    assert used == set(_abi.MOTION_MACROS) == {"HV_MOTION_TILE", "HV_MOTION_MAX_RADIUS", "HV_MOTION_MAX_LAM"}
    assert _abi.MOTION_MACROS == {"HV_MOTION_TILE": 32, "HV_MOTION_MAX_RADIUS": 32, "HV_MOTION_MAX_LAM": 255}
    # nothing of this header leaks into the others: the main header's declarations, constants and version are the recorded ABI's
    for other in (_abi.DECLS, _abi.CONTENT_DECLS, _abi.TEMPORAL_DECLS, _abi.GSSIM_DECLS, _abi.YUVW_DECLS):
        assert not {n for _, n, _ in _abi.MOTION_DECLS} & {n for _, n, _ in other}
    assert not set(_abi.MOTION_MACROS) & set(_abi.MACROS)
    # the ctypes table against the signature typed in by hand
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    pins = {"hv_block_motion": ([p, l, l, l, i, i, i, i, i, i, i, i, i, i, i, i, i, p, p, p, p], i)}
    assert set(pins) == set(_lib.MOTION_SIGNATURES)
    lib = _lib.load()
    for name, (argtypes, restype) in pins.items():
        assert _lib.MOTION_SIGNATURES[name] == argtypes and _lib.MOTION_RESTYPES[name] is restype, name
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    hv = _lib.torch_ops()
    for name in pins:
        assert getattr(hv, name[len("hv_"):]).default._schema.name == "hv::" + name[len("hv_"):]


def test_generated_registration_source_is_up_to_date():
    spec = importlib.util.spec_from_file_location("gen_torch_ops", os.path.join(ROOT, "tools", "gen_torch_ops.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    text = g.gen(_abi.MOTION_DECLS, "hv_motion.h")
    assert open(g.MOTION_OUT).read() == text, "include/hv_motion.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 1
