"""Video tensors out as Motion-JPEG (csrc/hv_mjpeg.hip): device tensor [C,T,H,W] -> two kernels (measure, write) -> the entropy-coded
data of every frame on the device -> pinned staging -> an `.avi` of JPEG frames (`MJPG`: ffplay, mpv, VLC and every editor open it), or
one `.jpg` strip of evenly spaced frames for a figure.  And back in (csrc/hv_mjpeg_read.hip): `.avi` / `.jpg` -> pinned staging -> device
bytes -> three kernels (restart markers, Huffman decode, inverse DCT + chroma filter + colour) -> the clip [3,T,H,W] in [-1, 1].

The coder is baseline JPEG (ITU-T T.81) as include/hv_mjpeg.h states it: the 8-bit frames save_videos_grid would write (the quantiser of
utils/file_utils.py:frames_uint8), JFIF BT.601 colour, 4:2:0 chroma from 2 x 2 sums, an integer DCT, the Annex K tables under the IJG
quality rule, the Annex K Huffman tables without an optimisation pass, one restart interval per MCU row.  tests/mjpeg_ref.py restates it
byte for byte and tests/test_mjpeg_cpu.py anchors that restatement against libjpeg through Pillow.  The decoder is stated in
include/hv_mjpeg_read.h: baseline 4:2:0 frames with any Huffman tables and any restart interval, decoded to the bytes libjpeg's default
settings give (tests/mjpeg_read_ref.py restates it, tests/test_mjpeg_read_cpu.py compares that with Pillow).  JPEG only: no mp4, H.264,
4:4:4, progressive mode, audio or OpenDML (files stay below 2 GiB).  What is written can be read back: `read_mjpeg_clip` gives the clip
as a player shows it, `mjpeg_roundtrip` the same without leaving the card.  CPU tensors are refused like everywhere else in the package."""
from __future__ import annotations

import os
import re
import struct
from collections import namedtuple
from fractions import Fraction

import torch

from . import _abi, _lib

MAX_SIDE = _abi.MACROS["HV_YUV_MAX_SIDE"]
DEFAULT_QUALITY = _abi.MJPEG_MACROS["HV_MJPEG_DEFAULT_QUALITY"]
MCU = _abi.MJPEG_MACROS["HV_MJPEG_MCU"]
AVI_MAX_BYTES = 2 ** 31 - 1                # AVI 1.0
_CHUNK_BYTES = 64 << 20                    # of 8-bit RGB frames, the unit frames_per_chunk defaults to
_DTYPES = {torch.float16: 0, torch.float32: 1}
EOI = b"\xFF\xD9"

# T.81 Annex K.1 / K.2 in natural order
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# natural index of every zigzag position (T.81 Figure A.6)
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# T.81 Annex K.3 - K.6 as DHT segment bodies: Tc/Th, BITS, HUFFVAL
_AC_L = bytes.fromhex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
                      "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
                      "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_C = bytes.fromhex("0001020311040521310612415107617113223281081442" "91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738"
                      "393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6"
                      "a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
_DHT = ((0x00, bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
        (0x10, bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]), _AC_L),
        (0x01, bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
        (0x11, bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]), _AC_C))
assert all(sum(bits) == len(vals) for _, bits, vals in _DHT)


def _check_quality(quality):
    if int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"quality is a whole number 1 .. 100, got {quality!r}")
    return int(quality)


def quant_tables(quality: int):
    """(luminance, chrominance), 64 steps each in natural order: Annex K scaled by the IJG quality rule"""
    quality = _check_quality(quality)
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (_K1, _K2))


def jpeg_header(W: int, H: int, quality: int = DEFAULT_QUALITY) -> bytes:
    """every byte of a frame in front of its entropy-coded data: SOI, APP0 JFIF 1.01, DQT x 2, SOF0 (true W and H, 4:2:0), DHT x 4, DRI
    (one restart interval per MCU row), SOS.  The same for all frames of a clip."""
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"sides 1 .. {MAX_SIDE}, got {W} x {H}")
    seg = lambda marker, body: struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body
    out = b"\xFF\xD8" + seg(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, q in enumerate(quant_tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(q[n] for n in _ZIGZAG))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, bits, vals in _DHT:
        out += seg(0xC4, bytes([tc]) + bits + vals)
    out += seg(0xDD, struct.pack(">H", (W + MCU - 1) // MCU))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def avi_rate(fps):
    """(dwRate, dwScale): the fraction closest to `fps` with a denominator up to 1001 (30000 / 1001 for 29.97...)"""
    if not fps > 0:
        raise ValueError(f"fps must be positive, got {fps}")
    r = Fraction(fps).limit_denominator(1001)
    return r.numerator, r.denominator


AVI_HEADER_BYTES = 224


def avi_file_bytes(n_frames: int, movi_bytes: int) -> int:
    """the size of the file; ValueError when it passes what AVI 1.0 holds"""
    total = AVI_HEADER_BYTES + movi_bytes + 8 + 16 * n_frames
    if total > AVI_MAX_BYTES:
        raise ValueError(f"an AVI 1.0 file holds up to {AVI_MAX_BYTES} bytes, this clip needs at least {total} (OpenDML is out of scope: "
                         "write it in parts)")
    return total


def avi_header(W: int, H: int, fps, n_frames: int, movi_bytes: int, max_frame_bytes: int) -> bytes:
    """the first AVI_HEADER_BYTES bytes of an AVI 1.0 file of `n_frames` JPEG frames: RIFF 'AVI ', LIST 'hdrl' (avih; one LIST 'strl' of
    strh vids / MJPG and a 24-bit BITMAPINFOHEADER with biCompression MJPG), and the head of LIST 'movi', whose `movi_bytes` of `00dc`
    chunks (each padded to even length) follow; `avi_index` comes last.  ValueError when the file would pass 2^31 - 1 bytes."""
    rate, scale = avi_rate(fps)
    total = avi_file_bytes(n_frames, movi_bytes)
    ck = lambda cc, body: cc + struct.pack("<I", len(body)) + body
    avih = struct.pack("<14I", (1000000 * scale + rate // 2) // rate, 0, 0, 0x10, n_frames, 0, 1, max_frame_bytes, W, H, 0, 0, 0, 0)
    strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, scale, rate, 0, n_frames, max_frame_bytes, -1, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = ck(b"LIST", b"hdrl" + ck(b"avih", avih) + ck(b"LIST", b"strl" + ck(b"strh", strh) + ck(b"strf", strf)))
    head = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
    assert len(head) == AVI_HEADER_BYTES
    return head


def avi_chunk(jpeg_len: int) -> bytes:
    """the 8 bytes in front of a frame in `movi`; a frame of odd length is followed by one zero byte"""
    return b"00dc" + struct.pack("<I", jpeg_len)


def avi_index(frame_bytes) -> bytes:
    """idx1: every frame a key frame, offsets counted from the `movi` tag"""
    out, pos = b"", 4
    for n in frame_bytes:
        out += b"00dc" + struct.pack("<III", 0x10, pos, n)
        pos += 8 + n + (n & 1)
    return b"idx1" + struct.pack("<I", len(out)) + out


def avi_file(jpegs, W: int, H: int, fps) -> bytes:
    """a whole file from complete JPEG frames held on the host (small clips, tests)"""
    sizes = [len(j) for j in jpegs]
    movi = b"".join(avi_chunk(len(j)) + j + (b"\0" if len(j) & 1 else b"") for j in jpegs)
    return avi_header(W, H, fps, len(jpegs), len(movi), max(sizes)) + movi + avi_index(sizes)


def _check_clip(x, who):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.HVKernelError(f"{who}: expected a GPU tensor (this package has no CPU path), got "
                                 f"{x.device if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dim() != 4 or x.shape[0] not in (1, 3) or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
        raise _lib.HVKernelError(f"{who}: expected a video [C,T,H,W] with C = 1 | 3 and T, H, W >= 1, got {tuple(x.shape)}")
    if x.dtype not in _DTYPES:
        raise _lib.HVKernelError(f"{who}: the kernel reads fp16 or fp32, got {x.dtype}")
    C, T, H, W = x.shape
    if max(W, H) > MAX_SIDE:
        raise ValueError(f"{who}: sides up to {MAX_SIDE}, got {W} x {H}")
    if x.stride(3) != 1 or min(x.stride()) < 0:
        raise _lib.HVKernelError(f"{who}: W must be contiguous and no stride negative, got strides {x.stride()}")
    return C, T, H, W


def clip_to_jpeg(x: torch.Tensor, quality: int = DEFAULT_QUALITY, rescale: bool = False):
    """x [C,T,H,W] fp16 / fp32 on the GPU (C = 1 | 3, W contiguous, any non-negative strides) -> (scan, frame_offsets, header):
    scan uint8 on the device, the entropy-coded data of all frames back to back; frame_offsets int64 [T + 1] on the device; header the
    bytes of jpeg_header.  Frame t as a file is header + scan[frame_offsets[t] : frame_offsets[t + 1]] + EOI.  rescale: x is in [-1, 1]
    (else in [0, 1]).  One synchronisation: the total size, which the prefix sum of the measured intervals gives, sizes `scan`."""
    scan, offsets, rows = _clip_to_intervals(x, quality, rescale, "clip_to_jpeg")
    return scan, offsets[::rows], jpeg_header(x.shape[3], x.shape[2], quality)


def _clip_to_intervals(x, quality, rescale, who):
    """-> (scan, offsets int64 [T * rows + 1] on the device, rows): interval u = (frame, MCU row) is scan[offsets[u] : offsets[u + 1]]"""
    quality = _check_quality(quality)
    C, T, H, W = _check_clip(x, who)
    rows = (H + MCU - 1) // MCU
    args = (x, _DTYPES[x.dtype], C, x.stride(0), x.stride(1), x.stride(2), T, H, W, int(bool(rescale)), quality)
    sizes = torch.empty(T * rows, dtype=torch.int32, device=x.device)
    _lib.call("mjpeg_measure", *args, sizes)
    offsets = torch.zeros(T * rows + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(sizes, 0, dtype=torch.int64, out=offsets[1:])
    scan = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=x.device)
    _lib.call("mjpeg_write", *args, offsets, scan)
    return scan, offsets, rows


def write_mjpeg_clip(x: torch.Tensor, path: str, fps=24, quality: int = DEFAULT_QUALITY, rescale: bool = False, frames_per_chunk=None) -> str:
    """x [C,T,H,W] on the GPU -> an `.avi` of JPEG frames; returns the path.  The clip is coded `frames_per_chunk` whole frames at a
    time (default: as many as hold 64 MiB of 8-bit RGB) and copied through at most two pinned staging buffers, written to the file only
    after the event behind their copy has passed; the sizes in the headers are patched in at the end.  AVI 1.0 only: a file that would
    pass 2^31 - 1 bytes raises ValueError and the partial file is removed."""
    if not path.endswith(".avi"):
        raise ValueError(f"write_mjpeg_clip writes .avi files, got {path!r}")
    quality = _check_quality(quality)
    avi_rate(fps)
    C, T, H, W = _check_clip(x, "write_mjpeg_clip")
    per = max(1, _CHUNK_BYTES // (W * H * 3)) if frames_per_chunk is None else int(frames_per_chunk)
    if per < 1:
        raise ValueError(f"frames_per_chunk must be >= 1, got {frames_per_chunk}")
    per = min(per, T)
    header = jpeg_header(W, H, quality)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sizes, movi_bytes = [], 0
    try:
        with torch.cuda.device(x.device), open(path, "wb") as f:
            stream = torch.cuda.current_stream(x.device)
            f.write(b"\0" * AVI_HEADER_BYTES)
            nbuf = 1 if per >= T else 2
            pinned = [None] * nbuf
            pending = [None] * nbuf                              # (frame offsets on the host, event) of the copy into pinned[b]

            def drain(b):
                nonlocal movi_bytes
                offs, event = pending[b]
                event.synchronize()
                view = memoryview(pinned[b].numpy())
                for k in range(len(offs) - 1):
                    n = len(header) + offs[k + 1] - offs[k] + len(EOI)
                    movi_bytes += 8 + n + (n & 1)
                    sizes.append(n)
                    avi_file_bytes(len(sizes), movi_bytes)
                    f.write(avi_chunk(n))
                    f.write(header)
                    f.write(view[offs[k]:offs[k + 1]])
                    f.write(EOI + b"\0" if n & 1 else EOI)
                pending[b] = None
            chunks = (T + per - 1) // per
            for i, t0 in enumerate(range(0, T, per)):
                b = i % nbuf
                if pending[b] is not None:
                    drain(b)
                scan, offs, _ = clip_to_jpeg(x[:, t0:t0 + per], quality, rescale)
                if pinned[b] is None or pinned[b].numel() < scan.numel():
                    pinned[b] = torch.empty(max(scan.numel(), 1), dtype=torch.uint8, pin_memory=True)
                pinned[b][:scan.numel()].copy_(scan, non_blocking=True)
                offs = offs.tolist()                             # after the copy was enqueued: the total was synchronised already
                event = torch.cuda.Event()
                event.record(stream)
                pending[b] = (offs, event)
            for i in range(max(0, chunks - nbuf), chunks):       # oldest first
                if pending[i % nbuf] is not None:
                    drain(i % nbuf)
            f.write(avi_index(sizes))
            f.seek(0)
            f.write(avi_header(W, H, fps, T, movi_bytes, max(sizes)))
    except ValueError:
        if os.path.exists(path):
            os.remove(path)
        raise
    return path


def strip_frames(T: int, n: int):
    """the indices of `n` evenly spaced frames of T: Python's round(i * (T - 1) / (n - 1)); n = 1 gives frame 0"""
    if n < 1 or n > T:
        raise ValueError(f"a strip of {n} frames cannot be cut from {T}")
    return [0] if n == 1 else [round(i * (T - 1) / (n - 1)) for i in range(n)]


def write_jpeg_strip(x: torch.Tensor, path: str, n: int = 8, quality: int = DEFAULT_QUALITY, rescale: bool = False) -> str:
    """`n` evenly spaced frames of x [C,T,H,W] side by side in one `.jpg`, composed on the device and coded by the kernels of the
    clip with T = 1; ValueError for n > T or a sheet wider than the largest side"""
    if not path.endswith((".jpg", ".jpeg")):
        raise ValueError(f"write_jpeg_strip writes .jpg files, got {path!r}")
    C, T, H, W = _check_clip(x, "write_jpeg_strip")
    idx = strip_frames(T, int(n))
    if len(idx) * W > MAX_SIDE:
        raise ValueError(f"a strip of {len(idx)} frames of width {W} is wider than {MAX_SIDE}")
    sheet = torch.cat([x[:, t:t + 1] for t in idx], dim=3)
    scan, _, header = clip_to_jpeg(sheet, quality, rescale)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header)
        f.write(memoryview(scan.cpu().numpy()))
        f.write(EOI)
    return path


def save_videos_mjpeg(videos: torch.Tensor, path: str, rescale: bool = False, n_rows: int = 1, fps=24, quality: int = DEFAULT_QUALITY) -> str:
    """the GPU route of save_videos_grid for `.avi` paths: [B,C,T,H,W] on the device -> the grid of video_io.video_grid -> Motion-JPEG;
    any grid size is legal"""
    from .video_io import video_grid
    grid = video_grid(videos, n_rows)
    if grid.dtype not in _DTYPES:
        grid = grid.float()
    return write_mjpeg_clip(grid, path, fps, quality, rescale)


def add_save_mjpeg_arguments(parser):
    parser.add_argument("--save-mjpeg", action="store_true", help="write every reconstruction as <name>.avi, Motion-JPEG coded on the "
                        "GPU (lossy; --mjpeg-input reads such files back); the rate is the input file's, else --fps, else 24")
    parser.add_argument("--save-quality", type=int, default=None, help=f"JPEG quality 1 .. 100 of --save-mjpeg (default {DEFAULT_QUALITY})")
    parser.add_argument("--save-strip", type=int, default=None, metavar="N", help="with --save-mjpeg: also <name>_strip.jpg, N evenly "
                        "spaced frames side by side")


def check_save_mjpeg_arguments(parser, args):
    """the refusals of the two flags that only mean something with --save-mjpeg; returns the quality to use"""
    if not args.save_mjpeg and args.save_quality is not None:
        parser.error("--save-quality needs --save-mjpeg")
    if not args.save_mjpeg and args.save_strip is not None:
        parser.error("--save-strip needs --save-mjpeg")
    if args.save_quality is not None and not 1 <= args.save_quality <= 100:
        parser.error(f"--save-quality is 1 .. 100, got {args.save_quality}")
    if args.save_strip is not None and args.save_strip < 1:
        parser.error(f"--save-strip is at least 1, got {args.save_strip}")
    return DEFAULT_QUALITY if args.save_quality is None else args.save_quality


def save_reconstruction_mjpeg(recon: torch.Tensor, out_dir: str, stem: str, fps=None, quality: int = DEFAULT_QUALITY, strip=None):
    """one reconstruction [C,T,H,W] in [-1, 1] -> <out_dir>/<stem>.avi (and <stem>_strip.jpg); returns the paths written"""
    out = [write_mjpeg_clip(recon, os.path.join(out_dir, stem + ".avi"), 24 if fps is None else fps, quality, rescale=True)]
    if strip is not None:
        out.append(write_jpeg_strip(recon, os.path.join(out_dir, stem + "_strip.jpg"), strip, quality, rescale=True))
    return out


# ------------------------------------------------------------------------------------------------ reading (include/hv_mjpeg_read.h)

HUFF_BYTES = _abi.MJPEG_READ_MACROS["HV_MJPEG_HUFF_BYTES"]
QUANT_BYTES = _abi.MJPEG_READ_MACROS["HV_MJPEG_QUANT_BYTES"]
RST_ORDER = _abi.MJPEG_READ_MACROS["HV_MJPEG_RST_ORDER"]
SYNC_MACROS = _abi.MJPEG_SYNC_MACROS
ENTROPY_CHOICES = ("auto", "serial", "sync")
# the entropy stage (stage B) of a group of frames: "serial" = one decoder per restart interval (hv_mjpeg_decode_coefs), "sync" = the
# self-synchronising workgroup per interval (hv_mjpeg_decode_coefs_sync, include/hv_mjpeg_sync.h), "auto" = sync when the group's mean
# interval (scan bytes / intervals) is at least SYNC_MIN_INTERVAL_BYTES, i.e. for frames without restart markers.  Both stages write the
# same bytes.  The two values are measured ones: profiles/metrics/bench_mjpeg_sync.json, DESIGN section 4.
SYNC_MIN_INTERVAL_BYTES = 2048
SYNC_SUB_BYTES = 256
STATUS_REASONS = {1: "the entropy-coded data ran out", 2: "no Huffman code matches", 3: "a coefficient index past 63",
                  4: "an unexpected marker inside the interval"}
# (W, H, quant, huff, Ri, scan_begin, scan_end): quant = (Y, chroma) of 64 steps in natural order; huff = ((BITS, HUFFVAL) of DC Y, AC Y,
# DC chroma, AC chroma); Ri in MCUs, 0 = none; the entropy-coded bytes are data[scan_begin:scan_end]
JpegFrame = namedtuple("JpegFrame", "W H quant huff Ri scan_begin scan_end")
_ANNEX_K_HUFF = tuple((tuple(bits), tuple(vals)) for _, bits, vals in _DHT)
_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)", 0xC5: "SOF5", 0xC6: "SOF6",
              0xC7: "SOF7", 0xC9: "SOF9 (arithmetic)", 0xCA: "SOF10 (arithmetic)", 0xCB: "SOF11", 0xCD: "SOF13", 0xCE: "SOF14", 0xCF: "SOF15"}
_NEXT_MARKER = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")          # inside entropy-coded data: not stuffing, not RSTm, not a fill byte


def parse_jpeg(data) -> JpegFrame:
    """The headers of one baseline 4:2:0 JPEG frame (bytes-like) -> JpegFrame.  ValueError, naming the marker, for everything outside
    the scope of include/hv_mjpeg_read.h: any SOF but SOF0, 12-bit samples, component counts and sampling factors other than 2x2 / 1x1 /
    1x1, 16-bit quantisation tables, a scan that is not the one interleaved scan of all three components, a second scan, DNL, DAC.
    APPn and COM segments are skipped and fill bytes (0xFF) in front of a marker tolerated.  A frame without DHT gets the Annex K
    tables, as Motion-JPEG players give it."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("not a JPEG frame: no SOI marker at its start")
    qt, ht, sof, Ri, pos = {}, {}, None, 0, 2
    while True:
        if pos >= n or d[pos] != 0xFF:
            raise ValueError(f"no marker at byte {pos} (the headers end without an SOS)")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise ValueError("the headers end inside a marker")
        m = d[pos]
        pos += 1
        if m == 0xD9:
            raise ValueError("EOI before any scan")
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if pos + 2 > n:
            raise ValueError(f"marker 0x{m:02X}: the segment length is cut off")
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2 or pos + L > n:
            raise ValueError(f"marker 0x{m:02X}: a segment of {L} bytes does not fit the frame")
        body = d[pos + 2:pos + L]
        pos += L
        if m in _SOF_NAMES:
            raise ValueError(f"{_SOF_NAMES[m]}: only baseline sequential DCT (SOF0) is decoded")
        if m == 0xCC:
            raise ValueError("DAC: arithmetic coding is not decoded")
        if m == 0xDC:
            raise ValueError("DNL: the number of lines must stand in the frame header")
        if m == 0xDB:
            i = 0
            while i < len(body):
                pq, tq = body[i] >> 4, body[i] & 15
                if pq != 0:
                    raise ValueError("DQT: 16-bit quantisation tables are not baseline")
                if tq > 3 or i + 65 > len(body):
                    raise ValueError("DQT: malformed table")
                nat = [0] * 64
                for k in range(64):
                    nat[_ZIGZAG[k]] = body[i + 1 + k]
                if min(nat) < 1:
                    raise ValueError("DQT: a quantisation step of 0")
                qt[tq] = tuple(nat)
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(body):
                if i + 17 > len(body):
                    raise ValueError("DHT: malformed table")
                tc, th = body[i] >> 4, body[i] & 15
                bits = tuple(body[i + 1:i + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or i + 17 + cnt > len(body):
                    raise ValueError("DHT: malformed table")
                ht[(tc, th)] = (bits, tuple(body[i + 17:i + 17 + cnt]))
                i += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("DRI: malformed segment")
            Ri = (body[0] << 8) | body[1]
        elif m == 0xC0:
            if sof is not None:
                raise ValueError("SOF0: a second frame header")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("SOF0: malformed segment")
            if body[0] != 8:
                raise ValueError(f"SOF0: {body[0]}-bit samples, only 8-bit is decoded")
            H, W, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if H == 0:
                raise ValueError("SOF0: 0 lines (DNL) is not decoded")
            if W < 1 or max(W, H) > MAX_SIDE:
                raise ValueError(f"SOF0: sides 1 .. {MAX_SIDE}, got {W} x {H}")
            comps = [(body[6 + 3 * c], body[7 + 3 * c], body[8 + 3 * c]) for c in range(nc)]
            if nc != 3:
                raise ValueError(f"SOF0: {nc} component{'s' if nc != 1 else ''} ({'gray' if nc == 1 else 'CMYK' if nc == 4 else 'unknown'}); "
                                 "only three (Y, Cb, Cr) are decoded")
            if [c[1] for c in comps] != [0x22, 0x11, 0x11]:
                raise ValueError("SOF0: sampling factors " + " ".join(f"{c[1] >> 4}x{c[1] & 15}" for c in comps) +
                                 "; only 4:2:0 (2x2 1x1 1x1) is decoded")
            if comps[1][2] != comps[2][2]:
                raise ValueError("SOF0: Cb and Cr with different quantisation tables")
            sof = (W, H, comps)
        elif m == 0xDA:
            if sof is None:
                raise ValueError("SOS before SOF0")
            W, H, comps = sof
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise ValueError("SOS: malformed segment")
            if body[0] != 3 or [body[1 + 2 * c] for c in range(3)] != [c[0] for c in comps]:
                raise ValueError(f"SOS: a scan of {body[0]} component{'s' if body[0] != 1 else ''}; only one interleaved scan of all three is decoded")
            if tuple(body[7:10]) != (0, 63, 0):
                raise ValueError("SOS: spectral selection or successive approximation (progressive) is not decoded")
            tabs = [body[2 + 2 * c] for c in range(3)]
            if tabs[1] != tabs[2]:
                raise ValueError("SOS: Cb and Cr with different Huffman tables")
            for tq in (comps[0][2], comps[1][2]):
                if tq not in qt:
                    raise ValueError(f"SOS: quantisation table {tq} was never defined (DQT)")
            huff = []
            for t in (tabs[0], tabs[1]):
                for tc, th in ((0, t >> 4), (1, t & 15)):
                    if ht:
                        if (tc, th) not in ht:
                            raise ValueError(f"SOS: Huffman table {'AC' if tc else 'DC'} {th} was never defined (DHT)")
                        huff.append(ht[(tc, th)])
                    else:
                        if th > 1:
                            raise ValueError(f"SOS: Huffman table {th} without any DHT")
                        huff.append(_ANNEX_K_HUFF[2 * th + tc])
            nxt = _NEXT_MARKER.search(d, pos)
            end = n if nxt is None else nxt.start()
            if nxt is not None:
                after = d[nxt.start() + 1]
                if after == 0xDC:
                    raise ValueError("DNL: the number of lines must stand in the frame header")
                if after == 0xDA or after in (0xC4, 0xDB, 0xDD) or after == 0xC0:
                    raise ValueError("SOS: a second scan; only one scan is decoded")
                if after != 0xD9:
                    raise ValueError(f"marker 0x{after:02X} behind the scan")
            frame = JpegFrame(W, H, (qt[comps[0][2]], qt[comps[1][2]]), tuple(huff), Ri, pos, end)
            huff_list(frame.huff)          # raises for a table the kernel would refuse
            return frame
        # APPn, COM and every other segment: skipped


def huff_list(huff):
    """((BITS, HUFFVAL) x 4) -> the HV_MJPEG_HUFF_BYTES ints of hv_mjpeg_decode_coefs; ValueError for a table it refuses"""
    out = []
    for i, (bits, vals) in enumerate(huff):
        if len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256:
            raise ValueError(f"DHT: table {i} is malformed")
        code = 0
        for l in range(16):
            code += bits[l]
            if code > (2 << l):
                raise ValueError(f"DHT: the code lengths of table {i} are over-subscribed")
            code <<= 1
        if any((v & 15) > 10 if i & 1 else v > 11 for v in vals):
            raise ValueError(f"DHT: table {i} holds a symbol no baseline block has")
        out += list(bits) + list(vals) + [0] * (256 - len(vals))
    assert len(out) == HUFF_BYTES
    return out


def intervals_per_frame(W: int, H: int, Ri: int) -> int:
    mpf = ((W + MCU - 1) // MCU) * ((H + MCU - 1) // MCU)
    return 1 if Ri == 0 else (mpf + Ri - 1) // Ri


def _u32(b, o):
    return struct.unpack_from("<I", b, o)[0]


def parse_avi(path: str):
    """An AVI 1.0 file of JPEG frames -> (W, H, fps, [(offset, size)]): the byte range of every frame in the file, in display order.
    The rate is strh's dwRate / dwScale (an int when whole, else a Fraction).  Frames are the `##dc` / `##db` chunks of the first `vids`
    stream, whose handler or compression must be MJPG; other streams are skipped.  They come from idx1 when it is present and every
    entry points at a chunk of that name and size inside `movi`, otherwise from walking `movi` (LIST `rec ` nesting included, odd sizes
    padded).  A chunk of zero length (a dropped frame) repeats the frame before it.  OpenDML (AVIX, indx) and files above 2^31 - 1
    bytes raise ValueError."""
    size = os.path.getsize(path)
    if size > AVI_MAX_BYTES:
        raise ValueError(f"{path}: {size} bytes; AVI 1.0 ends at {AVI_MAX_BYTES} (OpenDML is out of scope)")
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"{path}: not a RIFF AVI file")
        riff_end = min(size, 8 + _u32(head, 4))
        if size >= riff_end + 12:
            f.seek(riff_end)
            more = f.read(12)
            if more[:4] == b"RIFF" and more[8:12] == b"AVIX":
                raise ValueError(f"{path}: OpenDML (AVIX) is out of scope")
        stream, video, W, H = -1, None, 0, 0
        fps, movi, idx1 = None, None, None
        pos = 12
        while pos + 8 <= riff_end:
            f.seek(pos)
            cc, n = struct.unpack("<4sI", f.read(8))
            if cc == b"LIST":
                kind = f.read(4)
                if kind == b"hdrl":
                    hdrl = f.read(n - 4)
                    p = 0
                    while p + 8 <= len(hdrl):
                        c2, n2 = struct.unpack_from("<4sI", hdrl, p)
                        if c2 == b"LIST" and hdrl[p + 8:p + 12] == b"strl":
                            stream += 1
                            q, strh, strf = p + 12, None, None
                            while q + 8 <= p + 8 + n2:
                                c3, n3 = struct.unpack_from("<4sI", hdrl, q)
                                if c3 == b"strh":
                                    strh = hdrl[q + 8:q + 8 + n3]
                                elif c3 == b"strf":
                                    strf = hdrl[q + 8:q + 8 + n3]
                                elif c3 == b"indx":
                                    raise ValueError(f"{path}: OpenDML (indx) is out of scope")
                                q += 8 + n3 + (n3 & 1)
                            if video is None and strh is not None and strh[:4] == b"vids":
                                if len(strh) < 28 or strf is None or len(strf) < 20:
                                    raise ValueError(f"{path}: the video stream's strh / strf are cut short")
                                if strh[4:8].upper() != b"MJPG" and strf[16:20].upper() != b"MJPG":
                                    raise ValueError(f"{path}: the video stream is {strh[4:8]!r} / {strf[16:20]!r}, not MJPG")
                                scale, rate = _u32(strh, 20), _u32(strh, 24)
                                if scale == 0 or rate == 0:
                                    raise ValueError(f"{path}: strh has the rate {rate} / {scale}")
                                r = Fraction(rate, scale)
                                fps = r.numerator if r.denominator == 1 else r
                                W, H = struct.unpack_from("<ii", strf, 4)
                                video = stream
                        p += 8 + n2 + (n2 & 1)
                elif kind == b"movi":
                    movi = (pos + 8, pos + 8 + n)             # of the `movi` tag, behind the list
            elif cc == b"idx1":
                idx1 = (pos + 8, n)
            pos += 8 + n + (n & 1)
        if video is None or movi is None:
            raise ValueError(f"{path}: no MJPG video stream or no movi list")
        names = (b"%02ddc" % video, b"%02ddb" % video)
        movi_end = min(movi[1], size)
        frames = None
        if idx1 is not None and idx1[0] + idx1[1] <= size:
            f.seek(idx1[0])
            raw = f.read(idx1[1])
            ents = [struct.unpack_from("<4sIII", raw, i) for i in range(0, len(raw) - 15, 16)]
            mine = [(off, n) for cc, _, off, n in ents if cc in names]
            if mine:
                frames = []
                for base in (movi[0], 0):                      # offsets count from the movi tag, or (some writers) from the file start
                    frames = []
                    for off, n in mine:
                        at = base + off
                        f.seek(at)
                        hd = f.read(8)
                        if len(hd) < 8 or hd[:4] not in names or _u32(hd, 4) != n or at + 8 + n > movi_end or at < movi[0]:
                            frames = None
                            break
                        frames.append((at + 8, n))
                    if frames is not None:
                        break
        if frames is None:
            frames = []

            def walk(p, end):
                while p + 8 <= end:
                    f.seek(p)
                    cc, n = struct.unpack("<4sI", f.read(8))
                    if cc == b"LIST":
                        walk(p + 12, min(end, p + 8 + n))
                    elif cc in names:
                        if p + 8 + n > end:
                            break                              # a chunk cut off by the end of the file
                        frames.append((p + 8, n))
                    p += 8 + n + (n & 1)
            walk(movi[0] + 4, movi_end)
    out = []
    for off, n in frames:
        if n == 0:
            if not out:
                raise ValueError(f"{path}: the first frame is empty")
            out.append(out[-1])
        else:
            out.append((off, n))
    if not out:
        raise ValueError(f"{path}: no frames")
    if not (1 <= W <= MAX_SIDE and 1 <= abs(H) <= MAX_SIDE):
        raise ValueError(f"{path}: sides 1 .. {MAX_SIDE}, got {W} x {H}")
    return W, abs(H), fps, out


def _value_table(dtype, device, unit=False):
    """the 256 values a decoded byte becomes: dataset.yuv_value_table ([-1, 1], what a `.yuv` clip holds), or with `unit` q / 255 in
    fp32 cast to `dtype` ([0, 1], the floats compute_metrics makes of uint8 frames)"""
    from .dataset import _on, yuv_value_table
    if unit:
        return _on(("unit", dtype), device, lambda: (torch.arange(256, dtype=torch.uint8).float() / 255.0).to(dtype))
    return _on(("value", dtype), device, lambda: yuv_value_table(dtype))


def coef_bytes(T: int, H: int, W: int) -> int:
    return _lib.host("mjpeg_coef_bytes", T, H, W)


def _check_out(out, T, H, W, dtype, device, who):
    if out is None:
        if dtype not in _DTYPES:
            raise _lib.HVKernelError(f"{who}: the kernel writes fp16 or fp32, got {dtype}")
        return torch.empty(3, T, H, W, dtype=dtype, device=device)
    if not isinstance(out, torch.Tensor) or out.device != device or out.dtype not in _DTYPES or tuple(out.shape) != (3, T, H, W) or \
            (out.stride(3) != 1 and W > 1):
        raise _lib.HVKernelError(f"{who}: out must be a fp16 / fp32 [3,{T},{H},{W}] view on {device} with W contiguous, got "
                                 f"{getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    return out


def _check_entropy(entropy, sub_bytes, who):
    if entropy not in ENTROPY_CHOICES:
        raise ValueError(f"{who}: entropy is one of {', '.join(ENTROPY_CHOICES)}, got {entropy!r}")
    if sub_bytes is not None and not SYNC_MACROS["HV_MJPEG_SYNC_MIN_SUB"] <= int(sub_bytes) <= SYNC_MACROS["HV_MJPEG_SYNC_MAX_SUB"]:
        raise ValueError(f"{who}: sub_bytes is {SYNC_MACROS['HV_MJPEG_SYNC_MIN_SUB']} .. {SYNC_MACROS['HV_MJPEG_SYNC_MAX_SUB']}, got {sub_bytes!r}")
    return entropy, None if sub_bytes is None else int(sub_bytes)


def use_sync(entropy: str, scan_bytes: int, intervals: int) -> bool:
    """whether a group of frames with `scan_bytes` of entropy-coded data in `intervals` restart intervals takes the sync stage"""
    return entropy == "sync" or (entropy == "auto" and scan_bytes >= SYNC_MIN_INTERVAL_BYTES * intervals)


def _decode_group(data, begins, ends, frame, out, coefs, checks, unit=False, entropy="auto", sub_bytes=None):
    """stages A (when the frames carry restart markers), B and C for frames of equal parameters; appends (found, status, ipf) to checks"""
    T, dev = len(begins), data.device
    W, H, Ri = frame.W, frame.H, frame.Ri
    ipf = intervals_per_frame(W, H, Ri)
    b = torch.tensor(begins + ends, dtype=torch.int64).to(dev, non_blocking=True)
    ib, ie, found = b[:T], b[T:], None
    if ipf > 1:
        ib, ie = torch.empty(T * ipf, dtype=torch.int64, device=dev), torch.empty(T * ipf, dtype=torch.int64, device=dev)
        found = torch.empty(T, dtype=torch.int32, device=dev)
        _lib.call("mjpeg_find_restarts", data, data.numel(), b[:T], b[T:], T, ipf, ib, ie, found)
    sync = use_sync(entropy, sum(ends) - sum(begins), T * ipf)
    _decode_intervals(data, ib, ie, T, H, W, Ri, ipf, huff_list(frame.huff), list(frame.quant[0]) + list(frame.quant[1]), out, coefs,
                      checks, found, unit, sync, sub_bytes)


def _decode_intervals(data, ib, ie, T, H, W, Ri, ipf, huff, quant, out, coefs, checks, found=None, unit=False, sync=False, sub_bytes=None):
    need = coef_bytes(T, H, W)
    if coefs is None or coefs.numel() < need:
        coefs = torch.empty(need, dtype=torch.uint8, device=data.device)
    status = torch.empty(T * ipf, dtype=torch.int32, device=data.device)
    if sync:
        _lib.call("mjpeg_decode_coefs_sync", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, SYNC_SUB_BYTES if sub_bytes is None else sub_bytes,
                  coefs, coefs.numel(), status, None)
    else:
        _lib.call("mjpeg_decode_coefs", data, data.numel(), ib, ie, T, H, W, Ri, ipf, huff, coefs, coefs.numel(), status)
    _lib.call("mjpeg_coefs_to_clip", coefs, coefs.numel(), quant, _value_table(out.dtype, data.device, unit), out, _DTYPES[out.dtype],
              out.stride(0), out.stride(1), out.stride(2), T, H, W)
    checks.append((found, status, ipf))


def _raise_on_status(checks, path, first_frame):
    """one read-back of every found / status word of a call; ValueError(path, frame, interval, reason) on the first that is not clean"""
    flat = torch.cat([t.to(torch.int32).reshape(-1) for found, status, _ in checks for t in (found, status) if t is not None]).tolist()
    pos, frame = 0, first_frame
    for found, status, ipf in checks:
        T = status.numel() // ipf
        if found is not None:
            for t in range(T):
                v = flat[pos + t]
                if v != ipf - 1:
                    reason = "restart markers out of order" if v & RST_ORDER else f"{v & (RST_ORDER - 1)} restart markers, expected {ipf - 1}"
                    raise ValueError(path, frame + t, None, reason)
            pos += T
        for u in range(T * ipf):
            if flat[pos + u]:
                raise ValueError(path, frame + u // ipf, u % ipf, STATUS_REASONS.get(flat[pos + u], f"status {flat[pos + u]}"))
        pos += T * ipf
        frame += T


def jpeg_to_clip(data: torch.Tensor, frames, out: torch.Tensor = None, dtype=torch.float16, coefs: torch.Tensor = None, path=None,
                 first_frame: int = 0, unit: bool = False, checks: list = None, entropy: str = "auto", sub_bytes: int = None) -> torch.Tensor:
    """data: uint8 on the GPU holding the frames; frames: one JpegFrame per frame, its scan_begin / scan_end counted in `data` ->
    the clip [3,T,H,W] in [-1, 1] (channels R, G, B; `out`: a fp16 / fp32 view to fill, W contiguous, e.g. a frame slice of a larger
    clip).  Consecutive frames with equal parameters (size, tables, restart interval) are decoded by one launch of each stage; a file of
    write_mjpeg_clip is one group.  `coefs`: a uint8 workspace to reuse (coef_bytes).  The status words of all launches are read back
    once, at the end: ValueError(path, frame, interval, reason) for the first frame that did not decode (first_frame is added to the
    frame number); `out` then holds unspecified pixels.  checks: a list to which the status tensors of this call are appended INSTEAD of
    being read back, for a caller that makes several calls and reads them all once (read_mjpeg_clip; _raise_on_status).  unit: values byte / 255 in [0, 1] instead (compute_metrics' uint8 path).
    entropy, sub_bytes: the entropy stage of every group, see ENTROPY_CHOICES above (sub_bytes None: SYNC_SUB_BYTES); the result is the same."""
    entropy, sub_bytes = _check_entropy(entropy, sub_bytes, "jpeg_to_clip")
    if not isinstance(data, torch.Tensor) or not data.is_cuda or data.dtype != torch.uint8 or not data.is_contiguous():
        raise _lib.HVKernelError("jpeg_to_clip: expected contiguous uint8 on the GPU (this package has no CPU path), got "
                                 f"{(data.device, data.dtype) if isinstance(data, torch.Tensor) else type(data).__name__}")
    frames = list(frames)
    if not frames:
        raise ValueError("jpeg_to_clip: no frames")
    W, H = frames[0].W, frames[0].H
    for t, fr in enumerate(frames):
        if (fr.W, fr.H) != (W, H):
            raise ValueError(path, first_frame + t, None, f"a frame of {fr.W} x {fr.H} in a clip of {W} x {H}")
        if not 0 <= fr.scan_begin <= fr.scan_end <= data.numel():
            raise ValueError(path, first_frame + t, None, "the scan lies outside the data")
    out = _check_out(out, len(frames), H, W, dtype, data.device, "jpeg_to_clip")
    own, t0 = checks is None, 0
    checks = [] if own else checks
    with torch.cuda.device(data.device):
        while t0 < len(frames):
            t1 = t0 + 1
            while t1 < len(frames) and frames[t1][:5] == frames[t0][:5]:
                t1 += 1
            _decode_group(data, [f.scan_begin for f in frames[t0:t1]], [f.scan_end for f in frames[t0:t1]], frames[t0], out[:, t0:t1],
                          coefs, checks, unit, entropy, sub_bytes)
            t0 = t1
        if own:
            _raise_on_status(checks, path, first_frame)
    return out


def mjpeg_roundtrip(x: torch.Tensor, quality: int = DEFAULT_QUALITY, rescale: bool = False, dtype=None, entropy: str = "auto",
                    sub_bytes: int = None) -> torch.Tensor:
    """x [C,T,H,W] on the GPU -> [3,T,H,W] in [-1, 1]: the clip as a player of write_mjpeg_clip's file shows it, coded (clip_to_jpeg)
    and decoded again (stages B and C on the interval offsets the coder already has) without leaving the card.  entropy, sub_bytes: as
    jpeg_to_clip takes them (the coder's one interval per MCU row is what "auto" hands to the serial stage)."""
    entropy, sub_bytes = _check_entropy(entropy, sub_bytes, "mjpeg_roundtrip")
    scan, offsets, rows = _clip_to_intervals(x, quality, rescale, "mjpeg_roundtrip")
    C, T, H, W = x.shape
    out = _check_out(None, T, H, W, x.dtype if dtype is None else dtype, x.device, "mjpeg_roundtrip")
    if scan.numel() == 0:
        raise ValueError("mjpeg_roundtrip: the coder produced no data")
    q = quant_tables(quality)
    checks = []
    with torch.cuda.device(x.device):
        _decode_intervals(scan, offsets[:-1], offsets[1:], T, H, W, (W + MCU - 1) // MCU, rows, huff_list(_ANNEX_K_HUFF), q[0] + q[1], out,
                          None, checks, sync=use_sync(entropy, scan.numel(), T * rows), sub_bytes=sub_bytes)
        _raise_on_status(checks, None, 0)
    return out


def mjpeg_frame_range(n_frames: int, start=None, end=None):
    """(first frame, one behind the last) of [start, end) inside a file of n_frames"""
    first = 0 if start is None else max(0, int(start))
    last = n_frames if end is None else min(n_frames, int(end))
    return first, last


def read_mjpeg_clip(path: str, device="cuda", start=None, end=None, dtype=torch.float16, frames_per_chunk=None, unit: bool = False,
                    entropy: str = "auto", sub_bytes: int = None):
    """One Motion-JPEG `.avi` -> (clip [3,T,H,W] on `device` in [-1, 1], fps): the frames [start, end) of parse_avi.  The file is read
    `frames_per_chunk` whole frames at a time (default: as many as decode to 64 MiB of 8-bit RGB) into at most two pinned staging
    buffers; each chunk is uploaded with non_blocking=True and decoded straight into its frame slice of the output, a staging buffer is
    refilled only after the event behind its upload has passed, and the coefficient workspace is sized for one chunk (the kernels of
    consecutive chunks share it in stream order).  Nothing is synchronised between chunks: the host reads and parses chunk i + 1 while
    the device decodes chunk i, and the status words of all chunks are read back once, behind the last.  The headers of
    every frame are parsed on the host (parse_jpeg); ValueError(path, frame, interval, reason) for a frame that does not decode.
    entropy, sub_bytes: the entropy stage, as jpeg_to_clip takes them; "auto" gives files without restart markers (Pillow's, ffmpeg's, a
    camera's) the self-synchronising stage and files of write_mjpeg_clip the serial one."""
    entropy, sub_bytes = _check_entropy(entropy, sub_bytes, "read_mjpeg_clip")
    W, H, fps, index = parse_avi(path)
    first, last = mjpeg_frame_range(len(index), start, end)
    T = last - first
    if T < 1:
        raise ValueError(f"{path}: no frame in [{start}, {end})")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HVKernelError(f"read_mjpeg_clip: expected a GPU device (this package has no CPU path), got {device}")
    per = max(1, _CHUNK_BYTES // (W * H * 3)) if frames_per_chunk is None else int(frames_per_chunk)
    if per < 1:
        raise ValueError(f"frames_per_chunk must be >= 1, got {frames_per_chunk}")
    per = min(per, T)
    index = index[first:last]
    with torch.cuda.device(device):
        clip = torch.empty(3, T, H, W, dtype=dtype, device=device)
        stream = torch.cuda.current_stream(device)
        nbuf = 1 if per >= T else 2
        pinned, staged, uploaded = [None] * nbuf, [None] * nbuf, [None] * nbuf
        coefs = torch.empty(coef_bytes(per, H, W), dtype=torch.uint8, device=device)
        checks = []                                          # the status words of every chunk, read back once behind the last
        with open(path, "rb", buffering=0) as f:
            for i, t0 in enumerate(range(0, T, per)):
                part = index[t0:t0 + per]
                lo, hi = min(o for o, _ in part), max(o + n for o, n in part)
                b = i % nbuf
                if uploaded[b] is not None:
                    uploaded[b].synchronize()                # the upload that read this staging buffer is over
                if pinned[b] is None or pinned[b].numel() < hi - lo:
                    pinned[b] = torch.empty(hi - lo, dtype=torch.uint8, pin_memory=True)
                    staged[b] = torch.empty(hi - lo, dtype=torch.uint8, device=device)
                view = memoryview(pinned[b].numpy())[:hi - lo]
                f.seek(lo)
                got = 0
                while got < hi - lo:
                    k = f.readinto(view[got:])
                    if not k:
                        raise IOError(f"{path}: ended {hi - lo - got} bytes early (it shrank while being read)")
                    got += k
                frames = []
                for t, (o, n) in enumerate(part):
                    try:
                        fr = parse_jpeg(view[o - lo:o - lo + n])
                    except ValueError as e:
                        raise ValueError(path, first + t0 + t, None, str(e)) from e
                    if (fr.W, fr.H) != (W, H):
                        raise ValueError(path, first + t0 + t, None, f"a frame of {fr.W} x {fr.H} in a stream of {W} x {H}")
                    frames.append(fr._replace(scan_begin=fr.scan_begin + o - lo, scan_end=fr.scan_end + o - lo))
                staged[b][:hi - lo].copy_(pinned[b][:hi - lo], non_blocking=True)
                uploaded[b] = torch.cuda.Event()
                uploaded[b].record(stream)
                jpeg_to_clip(staged[b][:hi - lo], frames, out=clip[:, t0:t0 + len(part)], coefs=coefs, path=path, first_frame=first + t0,
                             unit=unit, checks=checks, entropy=entropy, sub_bytes=sub_bytes)
        for e in uploaded:
            if e is not None:
                e.synchronize()                              # the pinned buffers are freed on return
        _raise_on_status(checks, path, first)
    return clip, fps


def read_jpeg(path: str, device="cuda", dtype=torch.float16, entropy: str = "auto", sub_bytes: int = None) -> torch.Tensor:
    """One baseline 4:2:0 `.jpg` (a strip of write_jpeg_strip, or any such file) -> [3,1,H,W] on `device` in [-1, 1]; entropy,
    sub_bytes as jpeg_to_clip takes them"""
    entropy, sub_bytes = _check_entropy(entropy, sub_bytes, "read_jpeg")
    with open(path, "rb") as f:
        raw = f.read()
    try:
        fr = parse_jpeg(raw)
    except ValueError as e:
        raise ValueError(path, 0, None, str(e)) from e
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HVKernelError(f"read_jpeg: expected a GPU device (this package has no CPU path), got {device}")
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    return jpeg_to_clip(data, [fr], dtype=dtype, path=path, entropy=entropy, sub_bytes=sub_bytes)


def add_mjpeg_input_arguments(parser):
    parser.add_argument("--mjpeg-input", action="store_true", help="read --tensor-dir as a folder of Motion-JPEG .avi files (what "
                        "--save-mjpeg writes), decoded on the GPU, instead of .pt tensors; --start-frame / --end-frame select frames")
    parser.add_argument("--mjpeg-entropy", choices=ENTROPY_CHOICES, default=None, help="with --mjpeg-input: the entropy stage of the "
                        "decoder (default auto: the self-synchronising stage for files without restart markers, the serial one for "
                        "files --save-mjpeg wrote; the frames are the same)")
