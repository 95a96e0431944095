"""GPU: baseline JPEG frames -> video tensor (csrc/hv_mjpeg_read.hip through torch.ops.hv, the C ABI, mjpeg_io, the dataset and
compute_metrics) against the numpy restatement tests/mjpeg_read_ref.py, which tests/test_mjpeg_read_cpu.py holds to Pillow's decode.
Everything is integer arithmetic, so equality is BYTE-EXACT: the output is compared with vtab[reference bytes] by torch.equal, the
coefficient workspace and the status words with the restatement's.  The workspace, the status words and the interval offsets sit in
sentinel-filled buffers and the output is a strided view inside one; every cell outside must keep its value.  Dispatch edges of the
kernels: stage A walks strips of 256 x 16 = 4096 bytes; stage B runs 16 decoders per workgroup; stage C works on tiles of 4 x 2 MCUs
(64 x 32 pixels) with one chroma block around them, and switches the chroma filter off at W <= 4.  Corrupted input reaches the GPU only
in the two cases of test_corrupted_input_*: breadth is the job of the host fuzz program tools/mjpeg_decode_fuzz.cpp."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _lib, dataset, mjpeg_io  # noqa: E402
from tests import mjpeg_read_ref as D  # noqa: E402
from tests import mjpeg_ref as R  # noqa: E402
from tests.guarded_memory import GuardedFlat, crop, poisoned_vec  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mjpeg_read")
DTYPES = {torch.float16: 0, torch.float32: 1}
STRIP_BYTES, DECODERS, TILE = 4096, 16, (64, 32)


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _u8(values):
    return C.cast((C.c_uint8 * len(values))(*values), C.c_void_p)


class _Guarded64:
    """n int64 cells behind 16 bytes of sentinel and in front of 256 more (tests/guarded_memory.py has no 8-byte cells)"""

    def __init__(self, n):
        self.g = GuardedFlat(2 * n, torch.int32, front=4)
        self.view = self.g.view.view(torch.int64)

    def intact(self):
        return self.g.intact()


def _expected(ref_bytes: np.ndarray, dtype):
    """vtab[bytes] on the device"""
    return dataset.yuv_value_table(dtype).to(DEV)[torch.from_numpy(ref_bytes.astype(np.int64)).to(DEV)]


@functools.lru_cache(maxsize=None)
def _case(name, T):
    """-> tuple of T JPEG files of one size"""
    g = torch.Generator().manual_seed(500 + T)
    sizes = {"1x1": (1, 1, 75), "4x5": (4, 5, 75), "5x4": (5, 4, 75), "16x16": (16, 16, 75), "17x33": (17, 33, 75), "40x56_q100": (40, 56, 100),
             "16x160": (16, 160, 75)}
    W, H, q = sizes[name]
    return tuple(R.frames(torch.rand(3, T, H, W, generator=g), q))


@functools.lru_cache(maxsize=None)
def _reference(frames):
    """-> (uint8 [3,T,H,W], coefs int16 [T, rows, mcus, 6, 64], status lists, parsed frames)"""
    imgs, coefs, status = [], [], []
    for d in frames:
        p = D.parse(d)
        c, st, found = D.decode_coefs(d, p)
        assert found == D.geometry(p["W"], p["H"], p["Ri"])[3] - 1
        imgs.append(D.pixels(c, p["quant"], p["W"], p["H"])[0])
        coefs.append(c)
        status.append(st)
    return np.stack(imgs).transpose(3, 0, 1, 2), np.stack(coefs), status


def _stages(frames, dtype, route, ref=None, scan_ends=None):
    """the three stages on `frames` (JPEG files of equal parameters) with guarded buffers, twice; checks intervals, coefficients, status and
    pixels against the restatement and returns the status list.  scan_ends: per-frame ends of the scan to use instead of the parsed ones."""
    parsed = [mjpeg_io.parse_jpeg(d) for d in frames]
    assert all(p[:5] == parsed[0][:5] for p in parsed)
    fr = parsed[0]
    T, W, H, Ri = len(frames), fr.W, fr.H, fr.Ri
    ipf = mjpeg_io.intervals_per_frame(W, H, Ri)
    blob, begins, ends = b"", [], []
    for t, (d, p) in enumerate(zip(frames, parsed)):
        begins.append(len(blob) + p.scan_begin)
        ends.append(len(blob) + (p.scan_end if scan_ends is None else scan_ends[t]))
        blob += d
    data = poisoned_vec(torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV))
    sb, se = torch.tensor(begins, dtype=torch.int64, device=DEV), torch.tensor(ends, dtype=torch.int64, device=DEV)
    huff, quant = mjpeg_io.huff_list(fr.huff), list(fr.quant[0]) + list(fr.quant[1])
    need = mjpeg_io.coef_bytes(T, H, W)
    assert need == T * ((W + 15) // 16) * ((H + 15) // 16) * 768
    lib, stream = _lib.load(), _stream()
    # the restatement, on the same ranges
    ref_ib, ref_ie, ref_found, ref_status, ref_coefs = [], [], [], [], []
    for t, d in enumerate(frames):
        p = D.parse(d)
        ib, ie, found = D.find_restarts(blob, begins[t], ends[t], ipf)
        c, st, _ = D.decode_coefs(blob, dict(p, begin=begins[t], end=ends[t]))
        ref_ib += ib
        ref_ie += ie
        ref_found.append(found)
        ref_status += st
        ref_coefs.append(c)
    outs = []
    for run in range(2):
        gib, gie = _Guarded64(T * ipf), _Guarded64(T * ipf)
        gfound, gstatus = GuardedFlat(T, torch.int32, front=4), GuardedFlat(T * ipf, torch.int32, front=4)
        gcoefs = GuardedFlat(need // 2, torch.int16, front=16)
        buf, out, mask = crop((3, T, H, W), dtype, "out", poison=False)
        sentinel = buf.clone()
        if route == "ops":
            _lib.call("mjpeg_find_restarts", data, data.numel(), sb, se, T, ipf, gib.view, gie.view, gfound.view)
            _lib.call("mjpeg_decode_coefs", data, data.numel(), gib.view, gie.view, T, H, W, Ri, ipf, huff, gcoefs.view, need, gstatus.view)
            _lib.call("mjpeg_coefs_to_clip", gcoefs.view, need, quant, dataset.yuv_value_table(dtype).to(DEV), out, DTYPES[dtype], out.stride(0),
                      out.stride(1), out.stride(2), T, H, W)
        else:
            vtab = dataset.yuv_value_table(dtype).to(DEV)
            assert lib.hv_mjpeg_find_restarts(data.data_ptr(), data.numel(), sb.data_ptr(), se.data_ptr(), T, ipf, gib.view.data_ptr(),
                                              gie.view.data_ptr(), gfound.view.data_ptr(), stream) == 0
            assert lib.hv_mjpeg_decode_coefs(data.data_ptr(), data.numel(), gib.view.data_ptr(), gie.view.data_ptr(), T, H, W, Ri, ipf, _u8(huff),
                                             gcoefs.view.data_ptr(), need, gstatus.view.data_ptr(), stream) == 0
            assert lib.hv_mjpeg_coefs_to_clip(gcoefs.view.data_ptr(), need, _u8(quant), vtab.data_ptr(), out.data_ptr(), DTYPES[dtype],
                                              out.stride(0), out.stride(1), out.stride(2), T, H, W, stream) == 0
        torch.cuda.synchronize()
        assert gib.view.tolist() == ref_ib and gie.view.tolist() == ref_ie and gfound.view.tolist() == ref_found
        status = gstatus.view.tolist()
        assert status == ref_status
        assert torch.equal(gcoefs.view.cpu(), torch.from_numpy(np.stack(ref_coefs).reshape(-1)))
        for g in (gib, gie, gfound, gstatus, gcoefs):
            assert g.intact()
        assert torch.equal(buf[mask], sentinel[mask]), "a cell outside the output view was written"
        if not any(status):
            want = ref if ref is not None else D.decode_clip(frames)
            assert torch.equal(out, _expected(want, dtype))
        outs.append(buf.clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    return status


@pytest.mark.parametrize("T", (1, 3))
@pytest.mark.parametrize("name", ("1x1", "4x5", "5x4", "16x16", "17x33", "40x56_q100", "16x160"))
def test_sizes_byte_exact(name, T):
    frames = _case(name, T)
    ref = _reference(frames)[0]
    for dtype in DTYPES:
        for route in ("ops", "capi"):
            assert not any(_stages(frames, dtype, route, ref))


@pytest.mark.parametrize("name", sorted(R.census_inputs()))
def test_census_inputs_byte_exact(name):
    x, q = R.census_inputs()[name]
    frames = tuple(R.frames(x, q))
    ref = _reference(frames)[0]
    assert not any(_stages(frames, torch.float16, "ops", ref)) and not any(_stages(frames, torch.float32, "capi", ref))


@pytest.mark.parametrize("variant", ("plain", "optimize", "ri3", "rows1", "ri5"))
def test_fixtures_byte_exact(variant):
    """Pillow's files: optimised Huffman tables, no restart markers (one decoder per frame), Ri = one MCU row (ri3 and rows1 at 37 x 53
    are the same bytes: that row is 3 MCUs), and the two kinds whose intervals do not line up with MCU rows: ri3 at 53 x 37 (4 x 3 MCUs,
    intervals begin inside a row and span two) and ri5 at 37 x 53 (intervals of 5, 5 and 2 of 12 MCUs)"""
    names = sorted(f for f in os.listdir(GOLDEN) if f.startswith(variant + "_"))
    assert len(names) == {"ri3": 9, "ri5": 3}.get(variant, 6)
    crossing = 0
    for i, fname in enumerate(names):
        frames = (open(os.path.join(GOLDEN, fname), "rb").read(),)
        fr = mjpeg_io.parse_jpeg(frames[0])
        assert (fr.Ri == 0) == (variant in ("plain", "optimize")) and (variant != "ri3" or fr.Ri == 3) and (variant != "ri5" or fr.Ri == 5)
        mcus, ipf = (fr.W + 15) // 16, mjpeg_io.intervals_per_frame(fr.W, fr.H, fr.Ri)
        crossing += any((k * fr.Ri) % mcus for k in range(ipf))
        assert not any(_stages(frames, (torch.float16, torch.float32)[i % 2], ("ops", "capi")[(i // 2) % 2]))
    assert crossing == {"ri3": 3, "ri5": 3}.get(variant, 0)             # files with an interval that begins inside an MCU row


def test_jpeg_to_clip_groups_frames_of_different_parameters():
    names = sorted(f for f in os.listdir(GOLDEN) if "_37x53_" in f)
    files = [open(os.path.join(GOLDEN, f), "rb").read() for f in names]
    files = files[:3] + files[:1] * 2 + files[3:]                       # a run of equal frames inside
    blob, frames, pos = b"", [], 0
    for d in files:
        p = mjpeg_io.parse_jpeg(d)
        frames.append(p._replace(scan_begin=p.scan_begin + pos, scan_end=p.scan_end + pos))
        blob += d
        pos += len(d)
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    ref = np.concatenate([D.decode_clip([d]) for d in files], axis=1)
    for dtype in DTYPES:
        assert torch.equal(mjpeg_io.jpeg_to_clip(data, frames, dtype=dtype), _expected(ref, dtype))
    with pytest.raises(ValueError, match="5 x 4"):
        small = mjpeg_io.parse_jpeg(open(os.path.join(GOLDEN, "plain_5x4_q75.jpg"), "rb").read())
        mjpeg_io.jpeg_to_clip(data, frames + [small])
    with pytest.raises(_lib.HVKernelError):
        mjpeg_io.jpeg_to_clip(data.cpu(), frames)


def test_find_restarts_alone():
    """stage A on bytes that need not decode: stuffed 0xFF 0x00 next to real markers, markers across the 16-byte chunks of a thread and
    the 4096-byte strips of a workgroup, a marker cut by the end of the range, more markers than intervals, fewer, and out of order"""
    rng = np.random.default_rng(21)
    body = bytearray(rng.integers(0, 0xD0, 3 * STRIP_BYTES + 100, dtype=np.uint8).tobytes())           # no 0xFF, no marker bytes
    for k, pos in enumerate((5, 15, 31, 32, STRIP_BYTES - 1, STRIP_BYTES + 16, 2 * STRIP_BYTES - 2, 2 * STRIP_BYTES + 200, 3 * STRIP_BYTES + 50)):
        body[pos:pos + 2] = bytes([0xFF, 0xD0 + k % 8])
    for pos in (3, 13, 47, STRIP_BYTES - 3, STRIP_BYTES + 1, 2 * STRIP_BYTES + 198):
        body[pos:pos + 2] = b"\xFF\x00"
    body[7:10] = b"\xFF\x00\xD1"                                                                       # 0x00 0xD1 is no marker
    small = bytes([1, 0xFF, 0x00, 0xFF, 0xD0, 2, 0xFF, 0x00, 0xD1, 0xFF, 0xD1, 3, 0xFF, 0xD3, 0xFF])
    blob = bytes(body) + small
    ranges = [(0, len(body)), (len(body), len(blob)), (len(body), len(body) + 4), (6, STRIP_BYTES), (40, 40)]
    data = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(DEV)
    sb = torch.tensor([r[0] for r in ranges], dtype=torch.int64, device=DEV)
    se = torch.tensor([r[1] for r in ranges], dtype=torch.int64, device=DEV)
    T = len(ranges)
    for ipf in (1, 3, 4, 10, 12):
        ref = [D.find_restarts(blob, b, e, ipf) for b, e in ranges]
        for route in ("ops", "capi"):
            gib, gie = _Guarded64(T * ipf), _Guarded64(T * ipf)
            gfound = GuardedFlat(T, torch.int32, front=4)
            if route == "ops":
                _lib.call("mjpeg_find_restarts", data, data.numel(), sb, se, T, ipf, gib.view, gie.view, gfound.view)
            else:
                assert _lib.load().hv_mjpeg_find_restarts(data.data_ptr(), data.numel(), sb.data_ptr(), se.data_ptr(), T, ipf, gib.view.data_ptr(),
                                                          gie.view.data_ptr(), gfound.view.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            assert gib.view.tolist() == sum((r[0] for r in ref), []), ipf
            assert gie.view.tolist() == sum((r[1] for r in ref), []), ipf
            assert gfound.view.tolist() == [r[2] for r in ref], ipf
            assert gib.intact() and gie.intact() and gfound.intact()
    n = D.find_restarts(blob, 0, len(body), 10)[2] & (D.RST_ORDER - 1)
    assert 7 <= n <= 9 and D.find_restarts(blob, 6, STRIP_BYTES, 10)[2] & (D.RST_ORDER - 1) >= 2       # the cases above are really there


def _clip(T=5, H=24, W=40, seed=9):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    base = torch.stack([(xx + 2 * t) % 32 / 31.0 for t in range(T)])[None].repeat(3, 1, 1, 1)
    return (base * 0.8 + 0.2 * torch.rand(3, T, H, W, generator=g)).float()


def test_read_mjpeg_clip_chunks_and_jpeg_to_clip(tmp_path):
    x = _clip()
    frames = R.frames(x, 80)
    path = str(tmp_path / "c.avi")
    open(path, "wb").write(mjpeg_io.avi_file(frames, x.shape[3], x.shape[2], 25))
    ref = D.decode_clip(frames)
    for dtype in DTYPES:
        whole, fps = mjpeg_io.read_mjpeg_clip(path, DEV, dtype=dtype)
        assert fps == 25 and whole.dtype == dtype and torch.equal(whole, _expected(ref, dtype))
        for per in (1, 2):
            assert torch.equal(mjpeg_io.read_mjpeg_clip(path, DEV, dtype=dtype, frames_per_chunk=per)[0], whole)
    part, _ = mjpeg_io.read_mjpeg_clip(path, DEV, start=1, end=4, frames_per_chunk=2)
    assert torch.equal(part, _expected(ref[:, 1:4], torch.float16))
    # the whole file on the device, the frames' ranges from the container
    raw = open(path, "rb").read()
    W, H, _, index = mjpeg_io.parse_avi(path)
    parsed = []
    for o, n in index:
        p = mjpeg_io.parse_jpeg(raw[o:o + n])
        parsed.append(p._replace(scan_begin=p.scan_begin + o, scan_end=p.scan_end + o))
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    assert torch.equal(mjpeg_io.jpeg_to_clip(data, parsed), _expected(ref, torch.float16))
    # into a frame slice of a larger clip
    big = torch.full((3, 9, H, W), 7.0, dtype=torch.float16, device=DEV)
    mjpeg_io.jpeg_to_clip(data, parsed, out=big[:, 2:7])
    assert torch.equal(big[:, 2:7], _expected(ref, torch.float16)) and bool((big[:, :2] == 7).all()) and bool((big[:, 7:] == 7).all())
    with pytest.raises(ValueError, match="no frame"):
        mjpeg_io.read_mjpeg_clip(path, DEV, start=5)
    # unit values: byte / 255, what compute_metrics makes of uint8 frames
    unit, _ = mjpeg_io.read_mjpeg_clip(path, DEV, dtype=torch.float32, unit=True)
    assert torch.equal(unit, (torch.from_numpy(ref).float() / 255.0).to(DEV))
    # the dataset and compute_metrics read the same clip
    ds = dataset.MjpegClipDataset(str(tmp_path), DEV)
    clip, name = ds[0]
    assert name == "c.avi" and ds.fps[name] == 25 and torch.equal(clip, _expected(ref, torch.float16))
    spec = importlib.util.spec_from_file_location("hvjr_cm", os.path.join(ROOT, "evaluation", "compute_metrics.py"))
    cm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cm)
    v, rescale = cm.read_video(path)
    assert rescale is False and torch.equal(v, unit)


@pytest.mark.parametrize("quality,rescale", [(90, False), (35, True), (100, False)])
def test_roundtrip_on_the_card_and_through_a_file(tmp_path, quality, rescale):
    x = _clip(T=3, H=33, W=50, seed=quality)
    if rescale:
        x = x * 2 - 1
    ref = D.decode_clip(R.frames(x, quality, rescale))
    for dtype in DTYPES:
        xd = x.to(DEV, dtype)
        ref_d = ref if dtype == torch.float32 else D.decode_clip(R.frames(xd.cpu(), quality, rescale))
        rt = mjpeg_io.mjpeg_roundtrip(xd, quality, rescale)
        assert rt.dtype == dtype and torch.equal(rt, _expected(ref_d, dtype))
        path = mjpeg_io.write_mjpeg_clip(xd, str(tmp_path / f"r{DTYPES[dtype]}.avi"), 24, quality, rescale)
        back, fps = mjpeg_io.read_mjpeg_clip(path, DEV, dtype=dtype)
        assert fps == 24 and torch.equal(back, rt)
        assert torch.equal(mjpeg_io.read_mjpeg_clip(path, DEV, dtype=dtype, frames_per_chunk=2)[0], rt)
    strip = mjpeg_io.write_jpeg_strip(x.to(DEV), str(tmp_path / "s.jpg"), 3, quality, rescale)
    img = mjpeg_io.read_jpeg(strip, DEV, torch.float32)
    assert img.shape == (3, 1, 33, 150) and torch.equal(img, _expected(D.decode_clip([open(strip, "rb").read()]), torch.float32))


def _first_bad_flip(d, p, lo=None, hi=None, accept=lambda status, found: any(status)):
    """the first single-bit change in [lo, hi) (default: the second half of the scan) that leaves the frame parseable with the same scan
    and that the restatement answers with a (status list, found word) `accept` takes"""
    lo, hi = (p["begin"] + p["end"]) // 2 if lo is None else lo, p["end"] if hi is None else hi
    for pos in range(lo, hi):
        m = bytearray(d)
        m[pos] ^= 0x10
        m = bytes(m)
        try:
            q = D.parse(m)
            fr = mjpeg_io.parse_jpeg(m)
        except ValueError:
            continue                                     # the change made a marker: the parsers refuse the frame, nothing to decode
        if (q["begin"], q["end"]) == (p["begin"], p["end"]) == (fr.scan_begin, fr.scan_end):
            _, status, found = D.decode_coefs(m, q)
            if accept(status, found):
                return m
    raise AssertionError("no such change of one bit")


def test_corrupted_input_truncated():
    d = open(os.path.join(GOLDEN, "ri3_37x53_q75.jpg"), "rb").read()
    p = mjpeg_io.parse_jpeg(d)
    cut = (p.scan_begin + p.scan_end) // 2
    status = _stages((d,), torch.float16, "ops", scan_ends=[cut])
    assert D.NO_BYTES in status and status[0] == D.OK                  # _stages compared the list with the restatement's
    data = torch.frombuffer(bytearray(d), dtype=torch.uint8).to(DEV)
    with pytest.raises(ValueError) as e:
        mjpeg_io.jpeg_to_clip(data, [p._replace(scan_end=cut)], path="f.jpg", first_frame=7)
    path, frame, interval, reason = e.value.args
    assert (path, frame) == ("f.jpg", 7) and "restart markers" in reason and interval is None


def test_corrupted_input_changed_byte():
    """one changed bit in interval 2 of a four-interval frame whose intervals cross MCU rows: that interval's status alone is not 0, and
    jpeg_to_clip names frame and interval"""
    d = open(os.path.join(GOLDEN, "ri3_53x37_q75.jpg"), "rb").read()
    p = D.parse(d)
    ib, ie, found = D.find_restarts(d, p["begin"], p["end"], 4)
    assert found == 3
    bad = _first_bad_flip(d, p, ib[2], ie[2], lambda status, found: found == 3 and status[2] and not (status[0] or status[1] or status[3]))
    status = _stages((bad,), torch.float32, "capi")
    assert len(status) == 4 and status[:2] == [0, 0] and status[3] == 0 and status[2] in (D.NO_BYTES, D.NO_CODE, D.INDEX, D.MARKER)
    data = torch.frombuffer(bytearray(bad), dtype=torch.uint8).to(DEV)
    with pytest.raises(ValueError) as e:
        mjpeg_io.jpeg_to_clip(data, [mjpeg_io.parse_jpeg(bad)], path="g.jpg", first_frame=2)
    path, frame, interval, reason = e.value.args
    assert (path, frame, interval) == ("g.jpg", 2, 2) and reason == mjpeg_io.STATUS_REASONS[status[2]]
