"""GPU: the self-synchronising entropy stage (csrc/hv_mjpeg_sync.hip, include/hv_mjpeg_sync.h) against the serial stage B and the numpy
restatement tests/mjpeg_read_ref.py, BYTE for byte: coefficients and status words of every fixture of tests/golden/mjpeg_read and
tests/golden/mjpeg_sync at sub_bytes 16, 17, 64 and 4096 (several rounds; an odd length; a few subsequences; less than one), one frame
and three frames of different lengths in one launch, through torch.ops.hv and through the C ABI, with and without `iters`, every output
in a sentinel-filled buffer whose other cells must keep their value.  Then the Python surface: entropy="sync" and "auto" give what
entropy="serial" gives.  All sizes are those of the fixtures.  Corrupted input reaches the GPU only in the two cases the reader's tests
allow themselves (a truncated scan, one changed bit); breadth is the job of the host program tools/mjpeg_sync_check.cpp."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _abi, _lib, mjpeg_io  # noqa: E402
from tests import mjpeg_read_ref as D  # noqa: E402
from tests.guarded_memory import GuardedFlat, poisoned_vec  # noqa: E402
from tests.mjpeg_gpu_helpers import _first_bad_flip, _Guarded64, _stream, _u8  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ, SYNC = (os.path.join(ROOT, "tests", "golden", d) for d in ("mjpeg_read", "mjpeg_sync"))
FIXTURES = sorted(glob.glob(os.path.join(READ, "*.jpg")) + glob.glob(os.path.join(SYNC, "*.jpg")))
SUBS = (16, 17, 64, 4096)
LANES = _abi.MJPEG_SYNC_MACROS["HV_MJPEG_SYNC_LANES"]
# three frames of equal size, tables and restart interval, of different lengths
TRIPLES = ([tuple(os.path.join(READ, f"{v}_q{q}.jpg") for q in (35, 75, 95)) for v in ("plain_37x53", "ri3_37x53", "rows1_5x4", "ri3_53x37", "ri5_37x53")] +
           [tuple(os.path.join(SYNC, n) for n in ("noise_64x48_q100_s0.jpg", "flat_64x48.jpg", "noise_64x48_q100_s2.jpg"))])


@functools.lru_cache(maxsize=None)
def _file(path):
    return open(path, "rb").read()


@functools.lru_cache(maxsize=None)
def _reference(paths, scan_ends=None):
    """the restatement on the frames laid back to back -> (blob, begins, ends, interval begins, interval ends, status, coefs int16 flat)"""
    blob, begins, ends = b"", [], []
    for t, path in enumerate(paths):
        p = mjpeg_io.parse_jpeg(_file(path))
        begins.append(len(blob) + p.scan_begin)
        ends.append(len(blob) + (p.scan_end if scan_ends is None else scan_ends[t]))
        blob += _file(path)
    ib, ie, status, coefs = [], [], [], []
    for t, path in enumerate(paths):
        p = D.parse(_file(path))
        ipf = D.geometry(p["W"], p["H"], p["Ri"])[3]
        b, e, _ = D.find_restarts(blob, begins[t], ends[t], ipf)
        c, st, _ = D.decode_coefs(blob, dict(p, begin=begins[t], end=ends[t]))
        ib, ie, status = ib + b, ie + e, status + st
        coefs.append(c.astype(np.int16).reshape(-1))
    return blob, begins, ends, ib, ie, status, torch.from_numpy(np.concatenate(coefs))


def _both_stages(paths, sub, with_iters, route="ops", scan_ends=None, blob_override=None):
    """stage A, then the serial and the sync stage B on the same intervals, each into guarded buffers; compares both with each other and
    with the restatement and returns (status list, iters list or None)"""
    blob, begins, ends, ref_ib, ref_ie, ref_status, ref_coefs = _reference(paths, scan_ends)
    if blob_override is not None:
        blob = blob_override
    fr = mjpeg_io.parse_jpeg(_file(paths[0]))
    T, W, H, Ri = len(paths), fr.W, fr.H, fr.Ri
    ipf = mjpeg_io.intervals_per_frame(W, H, Ri)
    data = poisoned_vec(torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV))
    sb, se = torch.tensor(begins, dtype=torch.int64, device=DEV), torch.tensor(ends, dtype=torch.int64, device=DEV)
    huff = mjpeg_io.huff_list(fr.huff)
    need = mjpeg_io.coef_bytes(T, H, W)
    gib, gie, gfound = _Guarded64(T * ipf), _Guarded64(T * ipf), GuardedFlat(T, torch.int32, front=4)
    _lib.call("mjpeg_find_restarts", data, data.numel(), sb, se, T, ipf, gib.view, gie.view, gfound.view)
    serial_status, serial_coefs = GuardedFlat(T * ipf, torch.int32, front=4), GuardedFlat(need // 2, torch.int16, front=16)
    _lib.call("mjpeg_decode_coefs", data, data.numel(), gib.view, gie.view, T, H, W, Ri, ipf, huff, serial_coefs.view, need, serial_status.view)
    gstatus, gcoefs = GuardedFlat(T * ipf, torch.int32, front=4), GuardedFlat(need // 2, torch.int16, front=16)
    giters = GuardedFlat(T * ipf, torch.int32, front=4) if with_iters else None
    if route == "ops":
        _lib.call("mjpeg_decode_coefs_sync", data, data.numel(), gib.view, gie.view, T, H, W, Ri, ipf, huff, sub, gcoefs.view, need, gstatus.view,
                  giters.view if with_iters else None)
    else:
        assert _lib.load().hv_mjpeg_decode_coefs_sync(data.data_ptr(), data.numel(), gib.view.data_ptr(), gie.view.data_ptr(), T, H, W, Ri, ipf,
                                                      _u8(huff), sub, gcoefs.view.data_ptr(), need, gstatus.view.data_ptr(),
                                                      giters.view.data_ptr() if with_iters else None, _stream()) == 0
    torch.cuda.synchronize()
    if blob_override is None:
        assert gib.view.tolist() == ref_ib and gie.view.tolist() == ref_ie
        assert serial_status.view.tolist() == ref_status and torch.equal(serial_coefs.view.cpu(), ref_coefs)
    status = gstatus.view.tolist()
    assert status == serial_status.view.tolist()
    assert torch.equal(gcoefs.view, serial_coefs.view)
    for g in (gib, gie, gfound, gstatus, gcoefs, serial_status, serial_coefs) + ((giters,) if with_iters else ()):
        assert g.intact()
    iters = giters.view.tolist() if with_iters else None
    if with_iters:
        lens = [e - b for b, e in zip(gib.view.tolist(), gie.view.tolist())]
        for st, it, n in zip(status, iters, lens):
            rounds = ((n + sub - 1) // sub + LANES - 1) // LANES
            assert it == -1 if st else 1 <= it <= rounds * (LANES + 1), (st, it, n)
    return status, iters, gcoefs.buf.clone()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(os.path.dirname(p)) + "/" + os.path.basename(p) for p in FIXTURES])
def test_fixture_byte_exact(path):
    for i, sub in enumerate(SUBS):
        status, iters, _ = _both_stages((path,), sub, with_iters=i % 2 == 0, route="ops" if i < 2 else "capi")
        assert not any(status)


@pytest.mark.parametrize("paths", TRIPLES, ids=[os.path.basename(t[0]) for t in TRIPLES])
def test_three_frames_of_different_lengths(paths):
    for i, sub in enumerate(SUBS):
        status, iters, _ = _both_stages(paths, sub, with_iters=i % 2 == 1, route="capi" if i < 2 else "ops")
        assert not any(status)


def test_iters_and_two_runs():
    """several rounds at sub_bytes 16 (379 subsequences), one decode iteration where a unit is one subsequence; two runs give the same bits"""
    paths = (os.path.join(SYNC, "noise_64x48_q100_s0.jpg"),)
    a = _both_stages(paths, 16, True)
    b = _both_stages(paths, 16, True)
    assert a[1] == b[1] and a[1][0] >= 2 and torch.equal(a[2], b[2])
    assert _both_stages(paths, 4096, True)[1] in ([1], [2])                       # two subsequences: lane 1 decodes again unless it guessed right
    assert _both_stages((os.path.join(SYNC, "one_1x1.jpg"),), 16, True)[1] == [1]
    assert _both_stages((os.path.join(SYNC, "flat_64x48.jpg"),), 64, True)[1] == [1]


def test_corrupted_input_truncated():
    path = os.path.join(READ, "ri3_37x53_q75.jpg")
    p = mjpeg_io.parse_jpeg(_file(path))
    cut = (p.scan_begin + p.scan_end) // 2
    for sub in (16, 64):
        status, iters, _ = _both_stages((path,), sub, True, scan_ends=(cut,))
        assert D.NO_BYTES in status and status[0] == D.OK
        assert all((it == -1) == (st != 0) for st, it in zip(status, iters))


def test_corrupted_input_changed_byte():
    path = os.path.join(READ, "ri3_53x37_q75.jpg")
    d = _file(path)
    p = D.parse(d)
    ib, ie, found = D.find_restarts(d, p["begin"], p["end"], 4)
    bad = _first_bad_flip(d, p, ib[2], ie[2], lambda status, found: found == 3 and status[2] and not (status[0] or status[1] or status[3]))
    want = D.decode_coefs(bad, D.parse(bad))
    for sub in (16, 64):
        status, iters, buf = _both_stages((path,), sub, True, route="capi", blob_override=bad)
        assert status == want[1] and status[2] != 0 and [it == -1 for it in iters] == [False, False, True, False]
        front = 16
        assert torch.equal(buf[front:front + want[0].size].cpu(), torch.from_numpy(want[0].astype(np.int16).reshape(-1)))


# ---- the Python surface ----

def _avi(tmp_path, names, folder=SYNC):
    jpegs = [_file(os.path.join(folder, n)) for n in names]
    fr = mjpeg_io.parse_jpeg(jpegs[0])
    path = str(tmp_path / "clip.avi")
    open(path, "wb").write(mjpeg_io.avi_file(jpegs, fr.W, fr.H, 24))
    return path, jpegs


def _spy(monkeypatch):
    """the names of the stage-B ops that run"""
    seen, real = [], _lib.call

    def call(name, *args):
        if name.startswith("mjpeg_decode_coefs"):
            seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return seen


def test_read_mjpeg_clip_and_jpeg_to_clip(tmp_path, monkeypatch):
    # groups of different parameters in one file: standard tables, Pillow's own tables, standard tables again
    names = ["noise_64x48_q100_s0.jpg", "noise_64x48_q100_s2.jpg", "noise_64x48_q95opt_s2.jpg", "flat_64x48.jpg"]
    path, jpegs = _avi(tmp_path, names)
    seen = _spy(monkeypatch)
    want, fps = mjpeg_io.read_mjpeg_clip(path, DEV, entropy="serial")
    assert fps == 24 and want.shape == (3, 4, 48, 64) and set(seen) == {"mjpeg_decode_coefs"}
    del seen[:]
    for kw in (dict(), dict(sub_bytes=16), dict(frames_per_chunk=1, sub_bytes=4096), dict(dtype=torch.float32, unit=True)):
        ref = want if "dtype" not in kw else mjpeg_io.read_mjpeg_clip(path, DEV, entropy="serial", **kw)[0]
        del seen[:]
        got, _ = mjpeg_io.read_mjpeg_clip(path, DEV, entropy="sync", **kw)
        assert torch.equal(got, ref) and set(seen) == {"mjpeg_decode_coefs_sync"}, kw
    blob = b"".join(jpegs)
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    frames, at = [], 0
    for j in jpegs:
        fr = mjpeg_io.parse_jpeg(j)
        frames.append(fr._replace(scan_begin=fr.scan_begin + at, scan_end=fr.scan_end + at))
        at += len(j)
    assert torch.equal(mjpeg_io.jpeg_to_clip(data, frames, entropy="sync", sub_bytes=32), want)
    assert torch.equal(mjpeg_io.jpeg_to_clip(data, frames, entropy="serial"), want)
    # auto: above and below the threshold (mean interval lengths 6063.5, 3121 and 48 bytes here)
    for threshold, ops in ((1, {"mjpeg_decode_coefs_sync"}), (1 << 40, {"mjpeg_decode_coefs"}), (3000, {"mjpeg_decode_coefs_sync", "mjpeg_decode_coefs"})):
        monkeypatch.setattr(mjpeg_io, "SYNC_MIN_INTERVAL_BYTES", threshold)
        del seen[:]
        assert torch.equal(mjpeg_io.read_mjpeg_clip(path, DEV)[0], want) and set(seen) == ops, threshold
        assert torch.equal(mjpeg_io.jpeg_to_clip(data, frames, entropy="auto"), want)


def test_files_with_restart_markers_and_read_jpeg(tmp_path, monkeypatch):
    path, jpegs = _avi(tmp_path, ["ri5_37x53_q35.jpg", "ri5_37x53_q75.jpg", "ri5_37x53_q95.jpg"], READ)
    want = mjpeg_io.read_mjpeg_clip(path, DEV, entropy="serial")[0]
    assert torch.equal(mjpeg_io.read_mjpeg_clip(path, DEV, entropy="sync", sub_bytes=16)[0], want)
    assert torch.equal(mjpeg_io.read_mjpeg_clip(path, DEV)[0], want)
    for folder, name in ((SYNC, "ramp_80x64_q75.jpg"), (SYNC, "one_1x1.jpg"), (READ, "optimize_37x53_q95.jpg")):
        p = os.path.join(folder, name)
        ref = mjpeg_io.read_jpeg(p, DEV, entropy="serial")
        assert torch.equal(mjpeg_io.read_jpeg(p, DEV, entropy="sync"), ref) and torch.equal(mjpeg_io.read_jpeg(p, DEV, entropy="sync", sub_bytes=16), ref)
        assert torch.equal(mjpeg_io.read_jpeg(p, DEV), ref)


def test_roundtrip_on_the_card(monkeypatch):
    g = torch.Generator().manual_seed(77)
    x = torch.rand(3, 3, 40, 56, generator=g).to(DEV)
    want = mjpeg_io.mjpeg_roundtrip(x, 90, entropy="serial")
    seen = _spy(monkeypatch)
    assert torch.equal(mjpeg_io.mjpeg_roundtrip(x, 90, entropy="sync"), want) and seen == ["mjpeg_decode_coefs_sync"]
    assert torch.equal(mjpeg_io.mjpeg_roundtrip(x, 90, entropy="sync", sub_bytes=16), want)
    assert torch.equal(mjpeg_io.mjpeg_roundtrip(x, 90), want)
    for threshold, op in ((1, "mjpeg_decode_coefs_sync"), (1 << 40, "mjpeg_decode_coefs")):
        monkeypatch.setattr(mjpeg_io, "SYNC_MIN_INTERVAL_BYTES", threshold)
        del seen[:]
        assert torch.equal(mjpeg_io.mjpeg_roundtrip(x, 90), want) and seen == [op]
