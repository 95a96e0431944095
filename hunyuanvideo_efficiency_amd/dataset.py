"""Raw planar YUV 4:2:0 files as study inputs (csrc/hv_yuv.hip): `.yuv` file -> device bytes -> one kernel -> the clip tensor
[3,T,H,W] in [-1, 1] that the VAE and the scorers take.

The fork makes its `.pt` inputs with dataset_processor/yuv_tensor.py (raw BVI-HFR `.yuv`) and mp42tensor.py; both need cv2 and
torchvision, which this environment lacks.  Raw YUV is the one input format that needs no codec: colour conversion
(cv2.cvtColor(COLOR_YUV2BGR_I420 / YV12 / NV12) + COLOR_BGR2RGB), the optional resize and ToTensor + 2x - 1 are integer arithmetic
and two table lookups per pixel, restated in include/hv_kernels.h (hv_yuv420_to_clip).  UNPINNED RESTATEMENT: without cv2 none of it
can be checked by executing the fork; tests/test_yuv_cpu.py anchors the colour rule against the BT.601 float formula over all 2^24
triples and against known answers.  The resize is THIS PROJECT'S rule (2-tap bilinear, half-pixel centres, 11-bit coefficients, on
the 8-bit R, G, B), modelled on cv2.resize's default but not claimed equal to its bytes.  mp4 input (mp42tensor.py) and
video_bit_rate.py stay out of scope: they need a decoder / ffprobe.  CPU tensors are refused like everywhere else in the package."""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from . import _abi, _lib

YUV_FORMATS = {"I420": _abi.MACROS["HV_YUV_I420"], "YV12": _abi.MACROS["HV_YUV_YV12"], "NV12": _abi.MACROS["HV_YUV_NV12"]}
COEF_BITS = _abi.MACROS["HV_YUV_COEF_BITS"]
MAX_SIDE = _abi.MACROS["HV_YUV_MAX_SIDE"]
_DTYPES = {torch.float16: 0, torch.float32: 1}
_CHUNK_BYTES = 64 << 20        # default bound of one pinned staging buffer
_dev_tables = {}


def parse_yuv_name(name: str):
    """yuv_tensor.py:41-61: (fps, W, H) from the first `<n>fps` and the first `<w>x<h>` of a file name; ValueError if either is absent"""
    fps = re.search(r"(\d+)fps", name)
    res = re.search(r"(\d+)x(\d+)", name)
    if not fps or not res:
        raise ValueError(f"{name}: a raw YUV file name must carry its frame rate and size, like '60fps' and '1920x1080'")
    return float(fps.group(1)), int(res.group(1)), int(res.group(2))


Y4M_FRAME_MARK = b"FRAME\n"


def parse_y4m_header(line: bytes, name: str = "y4m"):
    """the stream header line of a YUV4MPEG2 file (without its newline) -> (fps, W, H).  Only 8-bit 4:2:0 (`C420*`; absent means 420jpeg)
    and progressive (`Ip`; absent is taken as progressive) streams are accepted; anything else raises a ValueError that names the token"""
    tokens = line.decode("ascii", "replace").split(" ")
    if tokens[0] != "YUV4MPEG2":
        raise ValueError(f"{name}: not a YUV4MPEG2 stream (it starts with {tokens[0][:16]!r})")
    W = H = fps = None
    for tok in tokens[1:]:
        if not tok:
            continue
        tag, val = tok[0], tok[1:]
        try:
            if tag == "W":
                W = int(val)
            elif tag == "H":
                H = int(val)
            elif tag == "F":
                num, den = val.split(":")
                fps = int(num) / int(den)
                if not fps > 0:
                    raise ValueError
        except (ValueError, ZeroDivisionError):
            raise ValueError(f"{name}: malformed header token {tok!r}") from None
        if tag == "C" and val not in ("420", "420jpeg", "420mpeg2", "420paldv"):      # C420p10 and friends are not 8-bit
            raise ValueError(f"{name}: only 8-bit 4:2:0 streams are read, the header says {tok!r}")
        if tag == "I" and val != "p":
            raise ValueError(f"{name}: only progressive streams are read, the header says {tok!r}")
    if W is None or H is None or fps is None:
        raise ValueError(f"{name}: the header lacks {'W' if W is None else 'H' if H is None else 'F'} ({line[:80]!r})")
    return fps, W, H


def read_y4m_header(path: str):
    """-> (fps, W, H, offset of the first FRAME marker)"""
    with open(path, "rb") as f:
        head = f.read(1024)
    end = head.find(b"\n")
    if end < 0:
        raise ValueError(f"{path}: no YUV4MPEG2 header line in the first {len(head)} bytes")
    return parse_y4m_header(head[:end], os.path.basename(path)) + (end + 1,)


def clip_file_info(path: str):
    """-> (fps, W, H, offset of the first frame record, bytes in front of every frame): a `.y4m` file says it in its header and has a
    `FRAME` line in front of every frame, a raw `.yuv` file in its name"""
    if path.endswith(".y4m"):
        return read_y4m_header(path) + (len(Y4M_FRAME_MARK),)
    return parse_yuv_name(os.path.basename(path)) + (0, 0)


def yuv_frame_bytes(W: int, H: int) -> int:
    if W < 2 or H < 2 or W % 2 or H % 2:
        raise ValueError(f"YUV 4:2:0 frames have even, positive sizes, got {W} x {H}")
    return W * H * 3 // 2


def yuv_frame_range(file_size: int, W: int, H: int, start=None, end=None):
    """yuv_tensor.py:95-104 -> (first frame, one behind the last): `end` None or behind the file is the count of WHOLE frames in the file
    (a truncated last frame is dropped), `start` None is 0, start >= end is empty (returned as (start, start))"""
    total = file_size // yuv_frame_bytes(W, H)
    if (start is not None and start < 0) or (end is not None and end < 0):
        raise ValueError(f"frame indices are non-negative, got start {start}, end {end}")
    end = total if end is None or end > total else end
    start = 0 if start is None else start
    return (start, end) if start < end else (start, start)


def target_size(W: int, H: int, target_height: int):
    """yuv_tensor.py:207-212 -> (width, height): the width keeps the aspect ratio in the host's double arithmetic, truncated, made even"""
    if target_height < 1:
        raise ValueError(f"target height must be positive, got {target_height}")
    return int(target_height * (W / H)) // 2 * 2, target_height


def resize_tables(src: int, dst: int) -> torch.Tensor:
    """One axis of the bilinear resize, int32 [dst, 2] on the host: entry d = (s, c1) - first source index, weight of the second index
    min(s + 1, src - 1) in COEF_BITS bits (c0 = 2^COEF_BITS - c1).  f = float32((d + 0.5) * (src / dst) - 0.5) with the product in double;
    s = floor(f), a = f - s in float32; outside [0, src - 1) s is clamped and a = 0; c1 = rint(a * 2^COEF_BITS), ties to even."""
    if src < 1 or dst < 1:
        raise ValueError(f"resize_tables: sizes must be positive, got {src} -> {dst}")
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * (src / dst) - 0.5).astype(np.float32)
    s = np.floor(f)
    a = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    out = (s < 0) | (s >= src - 1)
    s = np.clip(s, 0, src - 1)
    a[out] = np.float32(0)
    c1 = np.rint(a * np.float32(1 << COEF_BITS)).astype(np.int64)
    return torch.from_numpy(np.stack([s, c1], axis=1).astype(np.int32))


def yuv_value_table(dtype=torch.float16) -> torch.Tensor:
    """[256] in `dtype` on the host: entry q has the bits of (torch.tensor(q, dtype=uint8).float() / 255) * 2 - 1 - ToTensor, then
    2x - 1 (yuv_tensor.py:238,250) - and for fp16 that fp32 value cast once more, as infer.py casts a loaded .pt"""
    if dtype not in _DTYPES:
        raise _lib.HVKernelError(f"the YUV kernel writes fp16 or fp32, got {dtype}")
    return ((torch.arange(256, dtype=torch.uint8).float() / 255) * 2 - 1).to(dtype)


def _on(key, device, build):
    key = key + (torch.device(device),)
    if key not in _dev_tables:
        _dev_tables[key] = build().contiguous().to(device)
    return _dev_tables[key]


def yuv_to_clip(raw: torch.Tensor, W: int, H: int, fmt: str = "I420", out_dtype=torch.float16, size=None, out: torch.Tensor = None):
    """raw: uint8 GPU tensor of T whole frames (T * W * H * 3 / 2 contiguous bytes, any shape) in layout `fmt` -> [3,T,OH,OW] on the same
    device in [-1, 1], channels R, G, B.  `size` = (width, height) as `target_size` returns it (None: source size, no resize).  `out`: a
    [3,T,OH,OW] fp16 / fp32 view to fill instead (W contiguous; e.g. a frame slice of a larger clip).  Nothing is synchronised."""
    if fmt not in YUV_FORMATS:
        raise ValueError(f"yuv format is one of {sorted(YUV_FORMATS)}, got {fmt!r}")
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
        raise _lib.HVKernelError("yuv_to_clip: expected a GPU tensor (this package has no CPU path), got "
                                 f"{raw.device if isinstance(raw, torch.Tensor) else type(raw).__name__}")
    if raw.dtype != torch.uint8 or not raw.is_contiguous():
        raise _lib.HVKernelError(f"yuv_to_clip: raw frames are contiguous uint8, got {raw.dtype} with strides {raw.stride()}")
    frame = yuv_frame_bytes(W, H)
    if max(W, H) > MAX_SIDE:
        raise _lib.HVKernelError(f"yuv_to_clip: sides up to {MAX_SIDE}, got {W} x {H}")
    T = raw.numel() // frame
    if T < 1 or T * frame != raw.numel():
        raise _lib.HVKernelError(f"yuv_to_clip: {raw.numel()} bytes are not a whole number (>= 1) of {W} x {H} frames of {frame} bytes")
    OW, OH = (W, H) if size is None else (int(size[0]), int(size[1]))
    if OW < 1 or OH < 1 or max(OW, OH) > MAX_SIDE:
        raise _lib.HVKernelError(f"yuv_to_clip: output size {OW} x {OH} is outside [1, {MAX_SIDE}]")
    dev = raw.device
    if out is None:
        out = torch.empty(3, T, OH, OW, dtype=out_dtype, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev or out.dtype not in _DTYPES or tuple(out.shape) != (3, T, OH, OW) or \
            (out.stride(3) != 1 and OW > 1):
        raise _lib.HVKernelError(f"yuv_to_clip: out must be a fp16 / fp32 [3,{T},{OH},{OW}] view on {dev} with W contiguous, got "
                                 f"{getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))} strides {getattr(out, 'stride', lambda: ())()}")
    ytab = xtab = None
    if (OH, OW) != (H, W):
        ytab = _on(("axis", H, OH), dev, lambda: resize_tables(H, OH))
        xtab = _on(("axis", W, OW), dev, lambda: resize_tables(W, OW))
    vtab = _on(("value", out.dtype), dev, lambda: yuv_value_table(out.dtype))
    _lib.call("yuv420_to_clip", raw, T, YUV_FORMATS[fmt], W, H, out, _DTYPES[out.dtype], out.stride(0), out.stride(1), out.stride(2),
              OH, OW, ytab, xtab, vtab)
    return out


def read_yuv_clip(path: str, device="cuda", fmt: str = "I420", start=None, end=None, target_height=None, dtype=torch.float16,
                  frames_per_chunk=None):
    """One `.yuv` file -> (clip [3,T,OH,OW] on `device`, fps).  Size and frame rate come from the file name (`parse_yuv_name`), the frames
    [start, end) from `yuv_frame_range`; ValueError if no whole frame is in range.  A `.y4m` file (always I420: `fmt` must say so) carries
    size and rate in its header; the host drops its `FRAME` lines while staging, so the device sees the same bytes as for a `.yuv`.  The file is read `frames_per_chunk` whole frames at a
    time (default: as many as fit 64 MiB) into at most two pinned staging buffers, so host memory stays bounded whatever the file's
    length; each chunk is uploaded with non_blocking=True and converted straight into its frame slice of the output on the current
    stream, and a staging buffer is refilled only after the event behind its upload has passed."""
    fps, W, H, data0, mark = clip_file_info(path)
    if mark and fmt != "I420":
        raise ValueError(f"{path}: a .y4m file is I420, not {fmt}")
    frame = yuv_frame_bytes(W, H)
    first, last = yuv_frame_range((os.path.getsize(path) - data0) // (frame + mark) * frame, W, H, start, end)
    T = last - first
    if T < 1:
        raise ValueError(f"{path}: no whole frame in [{start}, {end})")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HVKernelError(f"read_yuv_clip: expected a GPU device (this package has no CPU path), got {device}")
    size = None if target_height is None else target_size(W, H, target_height)
    OW, OH = (W, H) if size is None else size
    per = max(1, _CHUNK_BYTES // frame) if frames_per_chunk is None else int(frames_per_chunk)
    if per < 1:
        raise ValueError(f"frames_per_chunk must be >= 1, got {frames_per_chunk}")
    per = min(per, T)
    with torch.cuda.device(device):
        clip = torch.empty(3, T, OH, OW, dtype=dtype, device=device)
        stream = torch.cuda.current_stream(device)
        nbuf = 1 if per >= T else 2
        pinned = [torch.empty(per * frame, dtype=torch.uint8, pin_memory=True) for _ in range(nbuf)]
        staged = [torch.empty(per * frame, dtype=torch.uint8, device=device) for _ in range(nbuf)]
        uploaded = [None] * nbuf
        with open(path, "rb", buffering=0) as f:
            f.seek(data0 + first * (frame + mark))
            for i, t0 in enumerate(range(0, T, per)):
                n = min(per, T - t0)
                b = i % nbuf
                if uploaded[b] is not None:
                    uploaded[b].synchronize()        # the upload that read this staging buffer is over
                view = memoryview(pinned[b].numpy())[:n * frame]
                got = 0
                while got < n * frame:
                    stop = n * frame
                    if mark:                             # a FRAME line in front of every frame: checked and dropped
                        if got % frame == 0:
                            line = f.read(mark)
                            if line != Y4M_FRAME_MARK:
                                raise ValueError(f"{path}: frame {first + t0 + got // frame} starts with {line!r}, not a bare FRAME line "
                                                 "(frame parameters are not read)")
                        stop = (got // frame + 1) * frame
                    k = f.readinto(view[got:stop])
                    if not k:
                        raise IOError(f"{path}: ended {n * frame - got} bytes early (it shrank while being read)")
                    got += k
                staged[b][:n * frame].copy_(pinned[b][:n * frame], non_blocking=True)
                uploaded[b] = torch.cuda.Event()
                uploaded[b].record(stream)
                yuv_to_clip(staged[b][:n * frame], W, H, fmt, size=size, out=clip[:, t0:t0 + n])
        for e in uploaded:
            if e is not None:
                e.synchronize()                      # the pinned buffers are freed on return
    return clip, fps


class YuvClipDataset:
    """The surface of infer.py's VideoTensorDataset over a folder of raw `.yuv` (and, for I420, `.y4m`) files: sorted names, `ds[i]` -> (clip [3,T,H,W] on the
    device, file name), with the fork's flags (yuv_tensor.py:16-24).  A file whose name does not parse or that has no whole frame in
    [start, end) is skipped with a printed line, as the fork skips it.  `fps[name]` holds each file's frame rate."""

    def __init__(self, video_dir, device="cuda", fmt="I420", start=None, end=None, target_height=None, dtype=torch.float16,
                 frames_per_chunk=None):
        if fmt not in YUV_FORMATS:
            raise ValueError(f"yuv format is one of {sorted(YUV_FORMATS)}, got {fmt!r}")
        self.tensor_dir, self.device, self.fmt, self.start, self.end = video_dir, device, fmt, start, end
        self.target_height, self.dtype, self.frames_per_chunk = target_height, dtype, frames_per_chunk
        self.tensor_files, self.fps, self.skipped = [], {}, []
        for name in sorted(f for f in os.listdir(video_dir) if f.endswith((".yuv", ".y4m"))):
            try:
                path = os.path.join(video_dir, name)
                fps, W, H, data0, mark = clip_file_info(path)
                if mark and fmt != "I420":
                    raise ValueError(f"a .y4m file is I420, not {fmt}")
                first, last = yuv_frame_range((os.path.getsize(path) - data0) // (yuv_frame_bytes(W, H) + mark) * yuv_frame_bytes(W, H),
                                              W, H, start, end)
            except ValueError as e:
                print(f"Skipping {name}: {e}")
                self.skipped.append(name)
                continue
            if last <= first:
                print(f"Skipping {name}: no whole frame in range")
                self.skipped.append(name)
                continue
            self.tensor_files.append(name)
            self.fps[name] = fps

    def __len__(self):
        return len(self.tensor_files)

    def __getitem__(self, idx):
        name = self.tensor_files[idx]
        clip, _ = read_yuv_clip(os.path.join(self.tensor_dir, name), self.device, self.fmt, self.start, self.end, self.target_height,
                                self.dtype, self.frames_per_chunk)
        return clip, name


class MjpegClipDataset:
    """The surface of YuvClipDataset over a folder of Motion-JPEG `.avi` files (what --save-mjpeg / write_mjpeg_clip write, or any AVI 1.0
    of baseline 4:2:0 JPEG frames): sorted names, `ds[i]` -> (clip [3,T,H,W] on the device in [-1, 1], file name), decoded on the GPU
    (mjpeg_io.read_mjpeg_clip).  A file that does not parse or has no frame in [start, end) is skipped with a printed line.
    `fps[name]` holds each file's frame rate."""

    def __init__(self, video_dir, device="cuda", start=None, end=None, dtype=torch.float16, frames_per_chunk=None, entropy="auto",
                 sub_bytes=None):
        from .mjpeg_io import _check_entropy, mjpeg_frame_range, parse_avi
        self.entropy, self.sub_bytes = _check_entropy(entropy, sub_bytes, "MjpegClipDataset")
        self.tensor_dir, self.device, self.start, self.end = video_dir, device, start, end
        self.dtype, self.frames_per_chunk = dtype, frames_per_chunk
        self.tensor_files, self.fps, self.skipped = [], {}, []
        for name in sorted(f for f in os.listdir(video_dir) if f.endswith(".avi")):
            try:
                W, H, fps, index = parse_avi(os.path.join(video_dir, name))
            except ValueError as e:
                print(f"Skipping {name}: {e}")
                self.skipped.append(name)
                continue
            first, last = mjpeg_frame_range(len(index), start, end)
            if last <= first:
                print(f"Skipping {name}: no frame in range")
                self.skipped.append(name)
                continue
            self.tensor_files.append(name)
            self.fps[name] = fps

    def __len__(self):
        return len(self.tensor_files)

    def __getitem__(self, idx):
        from .mjpeg_io import read_mjpeg_clip
        name = self.tensor_files[idx]
        clip, _ = read_mjpeg_clip(os.path.join(self.tensor_dir, name), self.device, self.start, self.end, self.dtype, self.frames_per_chunk,
                                  entropy=self.entropy, sub_bytes=self.sub_bytes)
        return clip, name


def add_yuv_arguments(parser):
    """--yuv-format and the flags valid only with it"""
    parser.add_argument("--yuv-format", choices=sorted(YUV_FORMATS), default=None, help="read --tensor-dir as a folder of raw planar YUV "
                        "4:2:0 files (<name>_<n>fps_<w>x<h>.yuv) in this layout, converted on the GPU, instead of .pt tensors")
    parser.add_argument("--target-height", type=int, default=None, help="with --yuv-format: resize to this many rows (width by aspect ratio, even)")
    parser.add_argument("--start-frame", type=int, default=None, help="with --yuv-format: first frame (inclusive)")
    parser.add_argument("--end-frame", type=int, default=None, help="with --yuv-format: last frame (exclusive)")


def check_yuv_arguments(args, parser):
    if getattr(args, "mjpeg_input", False):          # --mjpeg-input (mjpeg_io.add_mjpeg_input_arguments): frames may be selected, nothing else
        if args.yuv_format is not None:
            parser.error("--mjpeg-input and --yuv-format are two ways to read --tensor-dir: give one")
        if args.target_height is not None:
            parser.error("--target-height is only valid with --yuv-format")
        if (args.start_frame is not None and args.start_frame < 0) or (args.end_frame is not None and args.end_frame < 0):
            parser.error("--start-frame and --end-frame are non-negative")
        return
    if getattr(args, "mjpeg_entropy", None) is not None:
        parser.error("--mjpeg-entropy is only valid with --mjpeg-input")
    if args.yuv_format is None:
        for flag in ("target_height", "start_frame", "end_frame"):
            if getattr(args, flag) is not None:
                parser.error(f"--{flag.replace('_', '-')} is only valid with --yuv-format")
        return
    if args.target_height is not None and args.target_height < 1:
        parser.error("--target-height must be positive")
    if (args.start_frame is not None and args.start_frame < 0) or (args.end_frame is not None and args.end_frame < 0):
        parser.error("--start-frame and --end-frame are non-negative")


def dataset_from_args(args, device="cuda"):
    """the YuvClipDataset the flags of add_yuv_arguments ask for (fp16 clips, what the drivers feed the VAE); with --mjpeg-input the
    MjpegClipDataset"""
    if getattr(args, "mjpeg_input", False):
        return MjpegClipDataset(args.tensor_dir, device, args.start_frame, args.end_frame, entropy=getattr(args, "mjpeg_entropy", None) or "auto")
    return YuvClipDataset(args.tensor_dir, device, args.yuv_format, args.start_frame, args.end_frame, args.target_height)


def clip_stem(file_name: str) -> str:
    """the name a driver's outputs carry: the input file's stem"""
    return file_name[:-len(".yuv")] if file_name.endswith((".yuv", ".y4m", ".avi")) else file_name.replace(".pt", "")
