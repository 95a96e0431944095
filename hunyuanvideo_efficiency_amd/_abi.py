"""include/hv_kernels.h read once: the declarations of the C ABI and its integer `#define HV_*` constants.  Everything that has to
agree with the header (the ctypes table of _lib.py, the generated csrc/hv_torch_ops.cpp, the sizes ops.py / vae_ops.py / metrics.py
share with the kernels, tests/test_capi_cpu.py) takes it from here.  Standard library only."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hv_kernels.h")


class HVKernelError(RuntimeError):
    pass


def parse(text):
    """-> (decls, macros): decls = [(return C type, name, [(C type, parameter name), ...]), ...] in header order,
    macros = {"HV_...": int} of the `#define HV_* <integer>` lines."""
    macros = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^#define\s+(HV_\w+)\s+(\d\w*)\s*$", text, flags=re.M)}
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = []
    for m in re.finditer(r"\b(int|int64_t)\s+(hv_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = []
        if args not in ("", "void"):
            for a in args.split(","):
                pm = re.match(r"(.*?)(\w+)$", a.strip())
                params.append((pm.group(1).strip(), pm.group(2)))
        decls.append((ret, name, params))
    return decls, macros


if not os.path.exists(HEADER):
    raise HVKernelError(f"{HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout (the header is the one "
                        "description of the C ABI its bindings are derived from)")
with open(HEADER) as _f:
    DECLS, MACROS = parse(_f.read())

# include/hv_content.h: the content-statistics entry points (csrc/hv_content.hip), declared beside the main header, parsed the same way
CONTENT_HEADER = os.path.join(os.path.dirname(HEADER), "hv_content.h")
if not os.path.exists(CONTENT_HEADER):
    raise HVKernelError(f"{CONTENT_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(CONTENT_HEADER) as _f:
    CONTENT_DECLS, CONTENT_MACROS = parse(_f.read())

# include/hv_temporal.h: the linear temporal interpolation (csrc/hv_temporal.hip), declared and parsed the same way
TEMPORAL_HEADER = os.path.join(os.path.dirname(HEADER), "hv_temporal.h")
if not os.path.exists(TEMPORAL_HEADER):
    raise HVKernelError(f"{TEMPORAL_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(TEMPORAL_HEADER) as _f:
    TEMPORAL_DECLS, TEMPORAL_MACROS = parse(_f.read())

# include/hv_gssim.h: the Gaussian-window SSIM (csrc/hv_gssim.hip), declared and parsed the same way
GSSIM_HEADER = os.path.join(os.path.dirname(HEADER), "hv_gssim.h")
if not os.path.exists(GSSIM_HEADER):
    raise HVKernelError(f"{GSSIM_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(GSSIM_HEADER) as _f:
    GSSIM_DECLS, GSSIM_MACROS = parse(_f.read())

# include/hv_yuv_write.h: video tensor -> raw YUV 4:2:0 frames (csrc/hv_yuv_write.hip), declared and parsed the same way
YUVW_HEADER = os.path.join(os.path.dirname(HEADER), "hv_yuv_write.h")
if not os.path.exists(YUVW_HEADER):
    raise HVKernelError(f"{YUVW_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(YUVW_HEADER) as _f:
    YUVW_DECLS, YUVW_MACROS = parse(_f.read())

# include/hv_motion.h: block-matching motion fields (csrc/hv_motion.hip), declared and parsed the same way
MOTION_HEADER = os.path.join(os.path.dirname(HEADER), "hv_motion.h")
if not os.path.exists(MOTION_HEADER):
    raise HVKernelError(f"{MOTION_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(MOTION_HEADER) as _f:
    MOTION_DECLS, MOTION_MACROS = parse(_f.read())

# include/hv_mjpeg.h: video tensor -> baseline JPEG frames (csrc/hv_mjpeg.hip), declared and parsed the same way
MJPEG_HEADER = os.path.join(os.path.dirname(HEADER), "hv_mjpeg.h")
if not os.path.exists(MJPEG_HEADER):
    raise HVKernelError(f"{MJPEG_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(MJPEG_HEADER) as _f:
    MJPEG_DECLS, MJPEG_MACROS = parse(_f.read())

# include/hv_mjpeg_read.h: baseline JPEG frames -> video tensor (csrc/hv_mjpeg_read.hip), declared and parsed the same way
MJPEG_READ_HEADER = os.path.join(os.path.dirname(HEADER), "hv_mjpeg_read.h")
if not os.path.exists(MJPEG_READ_HEADER):
    raise HVKernelError(f"{MJPEG_READ_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(MJPEG_READ_HEADER) as _f:
    MJPEG_READ_DECLS, MJPEG_READ_MACROS = parse(_f.read())

# include/hv_mjpeg_sync.h: the self-synchronising entropy stage for frames without restart markers (csrc/hv_mjpeg_sync.hip), declared and
# parsed the same way
MJPEG_SYNC_HEADER = os.path.join(os.path.dirname(HEADER), "hv_mjpeg_sync.h")
if not os.path.exists(MJPEG_SYNC_HEADER):
    raise HVKernelError(f"{MJPEG_SYNC_HEADER} is missing: hunyuanvideo_efficiency_amd runs from a source checkout")
with open(MJPEG_SYNC_HEADER) as _f:
    MJPEG_SYNC_DECLS, MJPEG_SYNC_MACROS = parse(_f.read())
