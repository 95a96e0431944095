"""Video tensors out as raw YUV 4:2:0 (csrc/hv_yuv_write.hip): device tensor [C,T,H,W] -> one kernel -> device bytes -> pinned staging
-> a `.y4m` (YUV4MPEG2, opened by ffplay, mpv, VLC and every encoder) or a raw `.yuv` under the fork's naming
(`<stem>_<fps>fps_<W>x<H>.yuv`, read back by dataset.read_yuv_clip and by the fork's dataset_processor/yuv_tensor.py).

Raw YUV is the one output container that needs no codec.  The frames are the 8-bit frames save_videos_grid would write and every scorer
of metrics.py sees (the quantiser of utils/file_utils.py:frames_uint8), converted by the rule of include/hv_yuv_write.h: BT.601 limited
range in 20 fractional bits, chroma of a 2 x 2 block from its top-left pixel ("topleft", as OpenCV's COLOR_RGB2YUV_I420 does) or from the
four pixels' sums ("mean", THIS PROJECT'S rule and the default).  UNPINNED RESTATEMENT: cv2 cannot be executed here, so parity with its
bytes is not claimed; tests/test_yuv_write_cpu.py anchors the rule against the BT.601 float formula over all 2^24 triples and against
known answers.  mp4 or any codec, 10-bit, 4:2:2 / 4:4:4, BT.709 and a resize on the way out stay out of scope.  CPU tensors are refused
like everywhere else in the package."""
from __future__ import annotations

import os
import re
from fractions import Fraction

import torch

from . import _abi, _lib
from .dataset import _CHUNK_BYTES, MAX_SIDE, Y4M_FRAME_MARK, YUV_FORMATS, parse_yuv_name, yuv_frame_bytes

CHROMA_MODES = {"topleft": _abi.YUVW_MACROS["HV_YUVW_CHROMA_TOPLEFT"], "mean": _abi.YUVW_MACROS["HV_YUVW_CHROMA_MEAN"]}
SAVE_YUV_CHOICES = ("y4m", "I420", "YV12", "NV12")
_DTYPES = {torch.float16: 0, torch.float32: 1}


def _check_clip(x, who):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.HVKernelError(f"{who}: expected a GPU tensor (this package has no CPU path), got "
                                 f"{x.device if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dim() != 4 or x.shape[0] not in (1, 3) or x.shape[1] < 1:
        raise _lib.HVKernelError(f"{who}: expected a video [C,T,H,W] with C = 1 | 3 and T >= 1, got {tuple(x.shape)}")
    if x.dtype not in _DTYPES:
        raise _lib.HVKernelError(f"{who}: the kernel reads fp16 or fp32, got {x.dtype}")
    C, T, H, W = x.shape
    yuv_frame_bytes(W, H)                    # ValueError for odd or non-positive sizes
    if max(W, H) > MAX_SIDE:
        raise _lib.HVKernelError(f"{who}: sides up to {MAX_SIDE}, got {W} x {H}")
    if x.stride(3) != 1 or min(x.stride()) < 0:
        raise _lib.HVKernelError(f"{who}: W must be contiguous and no stride negative, got strides {x.stride()}")
    return C, T, H, W


def clip_to_yuv(x: torch.Tensor, fmt: str = "I420", rescale: bool = False, chroma: str = "mean", out: torch.Tensor = None):
    """x [C,T,H,W] fp16 / fp32 on the GPU (C = 1 | 3, W contiguous, any non-negative strides: an expanded view is fine) -> uint8
    [T, W*H*3/2] on the same device: T frames in layout `fmt`.  rescale: x is in [-1, 1] (else in [0, 1]), as save_videos_grid takes it.
    `out`: a contiguous uint8 tensor of T * W*H*3/2 elements to fill instead.  Nothing is synchronised."""
    if fmt not in YUV_FORMATS:
        raise ValueError(f"yuv format is one of {sorted(YUV_FORMATS)}, got {fmt!r}")
    if chroma not in CHROMA_MODES:
        raise ValueError(f"chroma is one of {sorted(CHROMA_MODES)}, got {chroma!r}")
    C, T, H, W = _check_clip(x, "clip_to_yuv")
    frame = yuv_frame_bytes(W, H)
    if out is None:
        out = torch.empty(T, frame, dtype=torch.uint8, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.device != x.device or out.dtype != torch.uint8 or out.numel() != T * frame or \
            not out.is_contiguous():
        raise _lib.HVKernelError(f"clip_to_yuv: out must be {T * frame} contiguous uint8 on {x.device}, got "
                                 f"{getattr(out, 'dtype', None)} {tuple(getattr(out, 'shape', ()))}")
    _lib.call("clip_to_yuv420", x, _DTYPES[x.dtype], C, x.stride(0), x.stride(1), x.stride(2), T, H, W, int(bool(rescale)),
              YUV_FORMATS[fmt], CHROMA_MODES[chroma], out)
    return out.view(T, frame)


def y4m_header(W: int, H: int, fps) -> bytes:
    """the stream header of a progressive 8-bit 4:2:0 file with square pixels; the rate as the fraction closest to `fps` with a
    denominator up to 1001 (30000:1001 for 30000 / 1001, 2997:100 for 29.97)"""
    if not fps > 0:
        raise ValueError(f"fps must be positive, got {fps}")
    r = Fraction(fps).limit_denominator(1001)
    return f"YUV4MPEG2 W{W} H{H} F{r.numerator}:{r.denominator} Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode("ascii")


def yuv_file_name(path: str, fps, W: int, H: int) -> str:
    """`path` (ending in .yuv) under the fork's naming: kept when its name already parses to (fps, W, H); else every `<n>fps` and
    `<w>x<h>` token is dropped from the stem and `_<fps>fps_<W>x<H>` appended.  The name holds whole rates only."""
    if fps != int(fps) or fps < 1:
        raise ValueError(f"a raw .yuv name carries a whole, positive frame rate, got {fps} (a .y4m header holds a fraction)")
    head, base = os.path.split(path)
    try:
        if parse_yuv_name(base) == (float(fps), W, H):
            return path
    except ValueError:
        pass
    stem = re.sub(r"_?\d+x\d+", "", re.sub(r"_?\d+fps", "", base[:-len(".yuv")]))
    return os.path.join(head, f"{stem}_{int(fps)}fps_{W}x{H}.yuv")


def write_yuv_clip(x: torch.Tensor, path: str, fps=24, fmt: str = None, rescale: bool = False, chroma: str = "mean", frames_per_chunk=None):
    """x [C,T,H,W] on the GPU -> a file; returns the path written.  `path` ends in `.y4m` (always I420; `fmt` None or "I420") or `.yuv`
    (layout `fmt`, default I420; the name as `yuv_file_name` makes it).  The clip is converted `frames_per_chunk` whole frames at a time
    (default: as many as fit 64 MiB) and copied through at most two pinned staging buffers, so host memory stays bounded whatever the
    clip's length; a staging buffer is written to the file, and reused, only after the event behind its copy has passed."""
    y4m = path.endswith(".y4m")
    if not y4m and not path.endswith(".yuv"):
        raise ValueError(f"write_yuv_clip writes .y4m or .yuv files, got {path!r}")
    if y4m and fmt not in (None, "I420"):
        raise ValueError(f"a .y4m file is always I420, got fmt {fmt!r}")
    fmt = "I420" if fmt is None else fmt
    if fmt not in YUV_FORMATS:
        raise ValueError(f"yuv format is one of {sorted(YUV_FORMATS)}, got {fmt!r}")
    if chroma not in CHROMA_MODES:
        raise ValueError(f"chroma is one of {sorted(CHROMA_MODES)}, got {chroma!r}")
    C, T, H, W = _check_clip(x, "write_yuv_clip")
    frame = yuv_frame_bytes(W, H)
    header = y4m_header(W, H, fps) if y4m else b""
    if not y4m:
        path = yuv_file_name(path, fps, W, H)
    per = max(1, _CHUNK_BYTES // frame) if frames_per_chunk is None else int(frames_per_chunk)
    if per < 1:
        raise ValueError(f"frames_per_chunk must be >= 1, got {frames_per_chunk}")
    per = min(per, T)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device)
        nbuf = 1 if per >= T else 2
        staged = torch.empty(per * frame, dtype=torch.uint8, device=x.device)       # stream order keeps one device buffer safe
        pinned = [torch.empty(per * frame, dtype=torch.uint8, pin_memory=True) for _ in range(nbuf)]
        pending = [None] * nbuf                                                     # (frames, event) of the copy into pinned[b]
        with open(path, "wb") as f:
            f.write(header)

            def drain(b):
                n, event = pending[b]
                event.synchronize()
                view = memoryview(pinned[b].numpy())
                if not y4m:
                    f.write(view[:n * frame])
                for k in range(n if y4m else 0):                 # a FRAME line in front of every frame
                    f.write(Y4M_FRAME_MARK)
                    f.write(view[k * frame:(k + 1) * frame])
                pending[b] = None
            for i, t0 in enumerate(range(0, T, per)):
                n = min(per, T - t0)
                b = i % nbuf
                if pending[b] is not None:
                    drain(b)
                clip_to_yuv(x[:, t0:t0 + n], fmt, rescale, chroma, out=staged[:n * frame])
                pinned[b][:n * frame].copy_(staged[:n * frame], non_blocking=True)
                event = torch.cuda.Event()
                event.record(stream)
                pending[b] = (n, event)
            chunks = (T + per - 1) // per
            for i in range(max(0, chunks - nbuf), chunks):                          # oldest first
                if pending[i % nbuf] is not None:
                    drain(i % nbuf)
    return path


def video_grid(videos: torch.Tensor, n_rows: int = 1, padding: int = 2) -> torch.Tensor:
    """utils/file_utils.py:_grid for every frame at once, on the device: [B,C,T,H,W] -> [C,T,GH,GW] (a view for B = 1)"""
    b, c, t, h, w = videos.shape
    if b == 1:
        return videos[0]
    xm = min(n_rows, b)
    ym = (b + xm - 1) // xm
    grid = torch.zeros(c, t, ym * (h + padding) + padding, xm * (w + padding) + padding, dtype=videos.dtype, device=videos.device)
    for k in range(b):
        y, x = (k // xm) * (h + padding) + padding, (k % xm) * (w + padding) + padding
        grid[:, :, y:y + h, x:x + w] = videos[k]
    return grid


def save_videos_yuv(videos: torch.Tensor, path: str, rescale: bool = False, n_rows: int = 1, fps=24, fmt: str = None, chroma: str = "mean"):
    """the GPU route of save_videos_grid: [B,C,T,H,W] on the device -> `.y4m` / `.yuv`; ValueError for an odd grid size"""
    grid = video_grid(videos, n_rows)
    if grid.shape[-1] % 2 or grid.shape[-2] % 2:
        raise ValueError(f"YUV 4:2:0 frames have even sizes, the grid is {grid.shape[-1]} x {grid.shape[-2]}")
    if grid.dtype not in _DTYPES:
        grid = grid.float()
    return write_yuv_clip(grid, path, fps, fmt, rescale, chroma)


def add_save_yuv_argument(parser):
    parser.add_argument("--save-yuv", choices=SAVE_YUV_CHOICES, default=None, help="write every reconstruction as 8-bit YUV 4:2:0, "
                        "converted on the GPU: y4m (YUV4MPEG2, any player) or a raw <name>_<n>fps_<w>x<h>.yuv in this layout, which "
                        "--yuv-format reads back; the rate is the input file's, else --fps, else 24")


def save_reconstruction(recon: torch.Tensor, out_dir: str, stem: str, save_yuv: str, fps=None) -> str:
    """one reconstruction [C,T,H,W] in [-1, 1] -> <out_dir>/<stem>.y4m or <out_dir>/<stem>_<fps>fps_<W>x<H>.yuv; returns the path"""
    fps = 24 if fps is None else fps
    if save_yuv == "y4m":
        return write_yuv_clip(recon, os.path.join(out_dir, stem + ".y4m"), fps, rescale=True)
    return write_yuv_clip(recon, os.path.join(out_dir, stem + ".yuv"), int(round(fps)), save_yuv, rescale=True)
