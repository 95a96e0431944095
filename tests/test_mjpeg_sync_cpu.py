"""CPU only: the self-synchronising entropy stage of include/hv_mjpeg_sync.h without a GPU.  tools/mjpeg_sync_check.cpp (the text the
kernel compiles, run lane by lane on the host) is built with the host compiler, without sanitizer flags, and run over the fixtures of
tests/golden/mjpeg_read and tests/golden/mjpeg_sync: it compares every unit with the serial decoder itself; here its coefficients and
status are held to the numpy restatement tests/mjpeg_read_ref.py as well, and its census lines must show every case the algorithm
distinguishes.  Then the refusals of the entry point from tests/mjpeg_sync_contract.py (skipped where a GPU is present: a missing guard
must never launch on made-up pointers), the bindings, the generated registration source, the Makefile, and the errors of the Python
surface."""
import ctypes as C
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from hunyuanvideo_efficiency_amd import _abi, _lib, mjpeg_io
from tests import mjpeg_read_ref as D
from tests import mjpeg_sync_contract as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mjpeg_read", "*.jpg")) +
                  glob.glob(os.path.join(ROOT, "tests", "golden", "mjpeg_sync", "*.jpg")))
SYNC_NAMES = {"noise_64x48_q100_s0.jpg": 6063, "noise_64x48_q100_s2.jpg": 6064, "noise_64x48_q95opt_s2.jpg": 3121, "flat_64x48.jpg": 48,
              "ramp_80x64_q75.jpg": 440, "one_1x1.jpg": 8, "ri3_37x53_q75.jpg": None, "rows1_53x37_q75.jpg": None}
no_gpu = pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: calls with made-up pointers must not reach a device")


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hvjs_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """-> (the program's output, the folder of its dumps at sub_bytes 16)"""
    out = tmp_path_factory.mktemp("mjpeg_sync_check")
    exe = str(out / "mjpeg_sync_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-I", os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "mjpeg_sync_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "--mutations=48", f"--dump={out}", "--dump-sub=16"] + FIXTURES, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout, str(out)


def _census(text):
    rows = []
    for line in text.splitlines():
        if line.startswith("census "):
            f = line.split()
            rows.append(dict({k: int(v) for k, v in (kv.split("=") for kv in f[2:])}, name=f[1]))
    return rows


def test_fixtures_are_what_the_generator_states():
    have = {os.path.basename(p) for p in FIXTURES if os.sep + "mjpeg_sync" + os.sep in p}
    assert have == set(SYNC_NAMES)
    for name, scan in SYNC_NAMES.items():
        d = open(os.path.join(ROOT, "tests", "golden", "mjpeg_sync", name), "rb").read()
        fr = mjpeg_io.parse_jpeg(d)
        assert scan is None or fr.scan_end - fr.scan_begin == scan, name
        assert (fr.Ri != 0) == name.startswith(("ri3", "rows1")), name
        assert len(d) < 8192


def test_census(program):
    """every case the algorithm distinguishes occurs in the unmutated fixtures (the fallback: in their mutations)"""
    text, _ = program
    rows = _census(text)
    subs = sorted({r["sub"] for r in rows})
    assert subs == list(range(16, 65)) + [128, 1024, 4096]
    assert {r["name"] for r in rows} == {os.path.basename(p) for p in FIXTURES}
    assert all(r["fallback"] == 0 for r in rows), "an unmutated fixture went through the serial decoder"
    at16 = {r["name"]: r for r in rows if r["sub"] == 16 and r["rst_inside"] == 0}
    s0 = at16["noise_64x48_q100_s0.jpg"]
    assert s0["scan"] == 6063 and s0["straddle"] == 4 and s0["rounds"] == 2                    # 379 subsequences of 16 bytes
    assert any(r["straddle"] > 0 for r in rows)                                                 # an FF 00 across a subsequence edge
    assert any(r["value_cross"] > 0 for r in rows)                                              # value bits across an edge
    assert any(r["span"] >= 3 for r in rows)                                                    # a block over >= 3 subsequences
    assert at16["flat_64x48.jpg"]["blocks"] >= 6 and any(r["blocks"] >= 6 for r in rows)        # >= 6 blocks inside one subsequence
    assert any(r["code"] > 9 for r in rows)                                                     # a code behind the 9-bit lookup
    assert any(r["rounds"] > 1 for r in rows) and at16["one_1x1.jpg"]["short"] == 1             # > 1 round; < 1 subsequence
    assert any(r["rst_end"] > 0 for r in rows) and any(r["rst_inside"] == 1 for r in rows)      # an interval that ends at an RSTm
    assert any(r["iters"] >= 2 for r in rows)                                                   # a round of >= 2 iterations
    assert at16["noise_64x48_q100_s2.jpg"]["scan"] % 16 == 0
    m = re.search(r"mjpeg_sync_check: (\d+) units compared with the serial decoder, (\d+) through the fallback, .* nothing differs", text)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 0                                # units that took the fallback


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(os.path.dirname(p)) + "/" + os.path.basename(p) for p in FIXTURES])
def test_program_equals_the_restatement(program, path):
    _, out = program
    d = open(path, "rb").read()
    coefs, status, _ = D.decode_coefs(d, D.parse(d))
    got = np.fromfile(os.path.join(out, os.path.basename(path) + ".coefs"), dtype=np.int16)
    assert got.tobytes() == coefs.astype(np.int16).tobytes()
    assert [int(v) for v in open(os.path.join(out, os.path.basename(path) + ".status")).read().split()] == status == [0] * len(status)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@no_gpu
@pytest.mark.parametrize("name,overrides,want", [pytest.param(n, ov, w, id=i) for i, n, ov, w in T.rows()])
def test_row(lib, name, overrides, want):
    """baseline: -2 (accepted, the launch fails without a device); refusal: -1; accept / last value inside a limit: -2"""
    assert T.call(lib, name, overrides) == want


@no_gpu
def test_the_refusals_the_issue_names(lib):
    for ov in (dict(sub_bytes=15), dict(sub_bytes=4097), dict(iters=T.PTR + 770)):
        assert T.call(lib, "hv_mjpeg_decode_coefs_sync", ov) == T.ARG
    for ov in (dict(sub_bytes=16), dict(sub_bytes=4096), dict(iters=None)):
        assert T.call(lib, "hv_mjpeg_decode_coefs_sync", ov) == T.LAUNCH


def test_the_table_covers_the_header_and_the_header_is_bound():
    decls = T.stream_decls()
    assert set(T.E) == set(decls) == {"hv_mjpeg_decode_coefs_sync"}
    e = T.E["hv_mjpeg_decode_coefs_sync"]
    params = decls["hv_mjpeg_decode_coefs_sync"]
    assert set(e.base) == {p for t, p in params if t != "hipStream_t"}
    assert sorted(e.required + e.nullable) == sorted(p for t, p in params if t.endswith("*"))
    assert _abi.MJPEG_SYNC_MACROS == {"HV_MJPEG_SYNC_LANES": 256, "HV_MJPEG_SYNC_MIN_SUB": 16, "HV_MJPEG_SYNC_MAX_SUB": 4096}
    # the reader's header is what it was
    assert {n for _, n, _ in _abi.MJPEG_READ_DECLS} == {"hv_mjpeg_coef_bytes", "hv_mjpeg_find_restarts", "hv_mjpeg_decode_coefs", "hv_mjpeg_coefs_to_clip"}
    # its parameters are those of hv_mjpeg_decode_coefs with sub_bytes and iters added
    serial = next(p for _, n, p in _abi.MJPEG_READ_DECLS if n == "hv_mjpeg_decode_coefs")
    assert [x for x in params if x[1] not in ("sub_bytes", "iters")] == serial
    p, i, l = C.c_void_p, C.c_int, C.c_int64
    want = [p, l, p, p, i, i, i, i, i, p, i, p, l, p, p, p]
    assert _lib.MJPEG_SYNC_SIGNATURES == {"hv_mjpeg_decode_coefs_sync": want} and _lib.MJPEG_SYNC_RESTYPES["hv_mjpeg_decode_coefs_sync"] is i
    fn = _lib.load().hv_mjpeg_decode_coefs_sync
    assert fn.argtypes == want and fn.restype is i
    hv = _lib.torch_ops()
    assert str(hv.mjpeg_decode_coefs_sync.default._schema) == (
        "hv::mjpeg_decode_coefs_sync(Tensor? data, int data_bytes, Tensor? interval_begin, Tensor? interval_end, int T, int H, int W, int Ri, "
        "int ipf, int[] huff_tables, int sub_bytes, Tensor(a!)? coefs, int coef_bytes, Tensor(b!)? status, Tensor(c!)? iters) -> ()")


def test_generated_registration_source_is_up_to_date():
    g = _load_script("tools/gen_torch_ops.py")
    text = g.gen(_abi.MJPEG_SYNC_DECLS, "hv_mjpeg_sync.h")
    assert open(g.MJPEG_SYNC_OUT).read() == text, "include/hv_mjpeg_sync.h changed: run python tools/gen_torch_ops.py"
    assert "TORCH_LIBRARY_FRAGMENT(hv, m)" in text and text.count("m.def(") == 1 and "huff_tables.size() == 1088" in text
    assert open(g.MJPEG_READ_OUT).read() == g.gen(_abi.MJPEG_READ_DECLS, "hv_mjpeg_read.h") and open(g.OUT).read() == g.gen()


def test_the_makefile_builds_and_links_the_new_sources():
    mk = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "Makefile")).read()
    assert "$(wildcard *.hip)" in mk and mk.count("hv_mjpeg_sync_torch_ops.cpp") == 2 and mk.count("../../include/hv_mjpeg_sync.h") == 2
    assert "hv_mjpeg_sync.hpp" in mk and "hv_wg_scan.hpp" in mk
    for name in ("hv_mjpeg_sync.hip", "hv_mjpeg_sync.hpp", "hv_wg_scan.hpp"):
        assert os.path.exists(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", name))
    hpp = open(os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_sync.hpp")).read()
    assert '#include "hv_mjpeg_decode.hpp"' in hpp


def test_python_errors(tmp_path):
    from hunyuanvideo_efficiency_amd import dataset
    assert mjpeg_io.ENTROPY_CHOICES == ("auto", "serial", "sync")
    assert T.MIN_SUB <= mjpeg_io.SYNC_SUB_BYTES <= T.MAX_SUB and mjpeg_io.SYNC_MIN_INTERVAL_BYTES >= 1
    with pytest.raises(ValueError, match="entropy"):
        mjpeg_io.jpeg_to_clip(None, [], entropy="bogus")
    with pytest.raises(ValueError, match="entropy"):
        mjpeg_io.read_mjpeg_clip(str(tmp_path / "none.avi"), entropy="bogus")
    with pytest.raises(ValueError, match="entropy"):
        mjpeg_io.read_jpeg(str(tmp_path / "none.jpg"), entropy="bogus")
    with pytest.raises(ValueError, match="entropy"):
        mjpeg_io.mjpeg_roundtrip(None, entropy="bogus")
    with pytest.raises(ValueError, match="entropy"):
        dataset.MjpegClipDataset(str(tmp_path), entropy="bogus")
    for bad in (15, 4097):
        with pytest.raises(ValueError, match="sub_bytes"):
            mjpeg_io.read_jpeg(str(tmp_path / "none.jpg"), entropy="sync", sub_bytes=bad)
    # auto: by the mean interval length
    n = mjpeg_io.SYNC_MIN_INTERVAL_BYTES
    assert mjpeg_io.use_sync("auto", 3 * n, 3) and not mjpeg_io.use_sync("auto", 3 * n - 1, 3)
    assert mjpeg_io.use_sync("sync", 0, 5) and not mjpeg_io.use_sync("serial", 1 << 30, 1)


@pytest.mark.parametrize("script,base", [("infer.py", ["--tensor-dir", "in", "--output-dir", "out"]),
                                         ("tools/run_vae_study.py", ["--tensor-dir", "in", "--output-dir", "out", "--base-config", "c.json"])])
def test_driver_arguments(script, base, capsys):
    mod = _load_script(script)
    assert mod.parse_args(base).mjpeg_entropy is None and mod.parse_args(base + ["--mjpeg-input"]).mjpeg_entropy is None
    for choice in mjpeg_io.ENTROPY_CHOICES:
        assert mod.parse_args(base + ["--mjpeg-input", "--mjpeg-entropy", choice]).mjpeg_entropy == choice
    for bad, msg in ((["--mjpeg-entropy", "sync"], "--mjpeg-entropy is only valid with --mjpeg-input"),
                     (["--yuv-format", "I420", "--mjpeg-entropy", "auto"], "--mjpeg-entropy is only valid with --mjpeg-input"),
                     (["--mjpeg-input", "--mjpeg-entropy", "bogus"], "invalid choice")):
        with pytest.raises(SystemExit):
            mod.parse_args(base + bad)
        assert msg in capsys.readouterr().err, bad
