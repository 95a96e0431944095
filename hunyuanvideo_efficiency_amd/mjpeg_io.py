"""Video tensors out as Motion-JPEG (csrc/hv_mjpeg.hip): device tensor [C,T,H,W] -> two kernels (measure, write) -> the entropy-coded
data of every frame on the device -> pinned staging -> an `.avi` of JPEG frames (`MJPG`: ffplay, mpv, VLC and every editor open it), or
one `.jpg` strip of evenly spaced frames for a figure.

The coder is baseline JPEG (ITU-T T.81) as include/hv_mjpeg.h states it: the 8-bit frames save_videos_grid would write (the quantiser of
utils/file_utils.py:frames_uint8), JFIF BT.601 colour, 4:2:0 chroma from 2 x 2 sums, an integer DCT, the Annex K tables under the IJG
quality rule, the Annex K Huffman tables without an optimisation pass, one restart interval per MCU row.  tests/mjpeg_ref.py restates it
byte for byte and tests/test_mjpeg_cpu.py anchors that restatement against libjpeg through Pillow.  JPEG only: no mp4, H.264, 4:4:4,
progressive mode, optimised Huffman tables, audio or OpenDML (files stay below 2 GiB); an `.avi` is written, never read back - the
lossy file is for people to look at, scores stay on the tensors.  CPU tensors are refused like everywhere else in the package."""
from __future__ import annotations

import os
import struct
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
    quality = _check_quality(quality)
    C, T, H, W = _check_clip(x, "clip_to_jpeg")
    rows = (H + MCU - 1) // MCU
    args = (x, _DTYPES[x.dtype], C, x.stride(0), x.stride(1), x.stride(2), T, H, W, int(bool(rescale)), quality)
    sizes = torch.empty(T * rows, dtype=torch.int32, device=x.device)
    _lib.call("mjpeg_measure", *args, sizes)
    offsets = torch.zeros(T * rows + 1, dtype=torch.int64, device=x.device)
    torch.cumsum(sizes, 0, dtype=torch.int64, out=offsets[1:])
    scan = torch.empty(int(offsets[-1]), dtype=torch.uint8, device=x.device)
    _lib.call("mjpeg_write", *args, offsets, scan)
    return scan, offsets[::rows], jpeg_header(W, H, quality)


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
                        "GPU (for people to look at: lossy, never read back); the rate is the input file's, else --fps, else 24")
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
