"""Bindings of the HIP extension.

* `libhv_kernels.so`   - the C ABI declared in include/hv_kernels.h (hipcc, gfx950).  `load()` binds it with ctypes: used by the
  symbol/ABI checks (tests/test_capi_cpu.py) and by any host that is not PyTorch.
* `libhv_torch_ops.so` - csrc/hv_torch_ops.cpp: TORCH_LIBRARY(hv, m) + TORCH_LIBRARY_IMPL(hv, CUDA, m), one custom op per C-ABI
  entry point (`torch.ops.hv.gemm_bf16`, `torch.ops.hv.attn_fwd_bf16`, ...), each launching on the current HIP stream of its
  tensors' device.  `call()` / `host()` are the product path: ops.py and vae_ops.py reach every kernel through torch.ops.hv.

There is NO fallback: if a shared library is missing or a symbol is absent the import of the compute path raises.  Build with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C hunyuanvideo_efficiency_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
import re

from . import _abi
from ._abi import HVKernelError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhv_kernels.so")
TORCH_OPS_PATH = os.path.join(_HERE, "lib", "libhv_torch_ops.so")
LOOP_INC = os.path.join(_HERE, "csrc", "hv_attention_w4_loop.inc")
ABI_VERSION = _abi.MACROS["HV_ABI_VERSION"]

_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "hipStream_t": C.c_void_p}


def _ctype(ctype: str, where: str):
    t = C.c_void_p if ctype.endswith("*") else _CTYPES.get(ctype)
    if t is None:
        raise HVKernelError(f"include/hv_kernels.h: {where}: no ctypes mapping for C type {ctype!r}")
    return t


# the header's declarations as ctypes: name -> argtypes, name -> restype
SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.DECLS}
RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.DECLS}
# the same for include/hv_content.h (same library, its own header)
CONTENT_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.CONTENT_DECLS}
CONTENT_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.CONTENT_DECLS}
# and for include/hv_temporal.h
TEMPORAL_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.TEMPORAL_DECLS}
TEMPORAL_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.TEMPORAL_DECLS}
# and for include/hv_gssim.h
GSSIM_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.GSSIM_DECLS}
GSSIM_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.GSSIM_DECLS}
# and for include/hv_yuv_write.h
YUVW_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.YUVW_DECLS}
YUVW_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.YUVW_DECLS}
# and for include/hv_motion.h
MOTION_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.MOTION_DECLS}
MOTION_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.MOTION_DECLS}
# and for include/hv_mjpeg.h
MJPEG_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.MJPEG_DECLS}
MJPEG_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.MJPEG_DECLS}
# and for include/hv_mjpeg_read.h
MJPEG_READ_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.MJPEG_READ_DECLS}
MJPEG_READ_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.MJPEG_READ_DECLS}
# and for include/hv_mjpeg_sync.h
MJPEG_SYNC_SIGNATURES = {name: [_ctype(t, f"{name}({p})") for t, p in params] for _, name, params in _abi.MJPEG_SYNC_DECLS}
MJPEG_SYNC_RESTYPES = {name: _ctype(ret, name) for ret, name, _ in _abi.MJPEG_SYNC_DECLS}
_lib = _hv = None       # the loaded ctypes handle / torch.ops.hv namespace


def loop_signature_in_tree():
    """HV_W4_LOOP_SIGNATURE of csrc/hv_attention_w4_loop.inc (the generated attention iteration); None if it carries none"""
    with open(LOOP_INC) as f:
        m = re.search(r"#define HV_W4_LOOP_SIGNATURE 0x([0-9a-f]{8})u", f.read(600))
    return None if m is None else int(m.group(1), 16)


def load():
    """Load (once) and return the ctypes handle; raises HVKernelError if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HVKernelError(
            f"{LIB_PATH} is missing: the HIP extension is not built (run __graft_entry__.build()). "
            "hunyuanvideo_efficiency_amd has no CPU or eager fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in list(SIGNATURES.items()) + list(CONTENT_SIGNATURES.items()) + list(TEMPORAL_SIGNATURES.items()) + \
            list(GSSIM_SIGNATURES.items()) + list(YUVW_SIGNATURES.items()) + list(MOTION_SIGNATURES.items()) + list(MJPEG_SIGNATURES.items()) + \
            list(MJPEG_READ_SIGNATURES.items()) + list(MJPEG_SYNC_SIGNATURES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HVKernelError(f"{LIB_PATH} does not export {name}") from e
        fn.argtypes = argtypes
        fn.restype = {**MJPEG_SYNC_RESTYPES, **MJPEG_READ_RESTYPES, **MJPEG_RESTYPES, **MOTION_RESTYPES, **YUVW_RESTYPES, **GSSIM_RESTYPES, **TEMPORAL_RESTYPES, **CONTENT_RESTYPES, **RESTYPES}[name]
    v = lib.hv_abi_version()
    if v != ABI_VERSION:
        raise HVKernelError(f"libhv_kernels ABI {v} != expected {ABI_VERSION}: rebuild the extension")
    # the attention kernel's steady-state iteration is generated code (csrc/hv_attention_w4_loop.inc): a library compiled from another
    # iteration - a stale file or a timing experiment's, which computes garbage by design - must not pass for the product
    if os.path.exists(LOOP_INC) and os.environ.get("HV_ALLOW_EXPERIMENT_LIB") != "1":
        if (lib.hv_attn_w4_loop_signature() & 0xFFFFFFFF) != loop_signature_in_tree():
            raise HVKernelError(f"{LIB_PATH} was not compiled from {LOOP_INC}: rebuild the extension (make -C hunyuanvideo_efficiency_amd/csrc); "
                                "HV_ALLOW_EXPERIMENT_LIB=1 admits a library built from another checkout (same-box A/Bs: tools/ab_attn.sh, tools/ab_run.sh)")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        raise HVKernelError(f"{what} failed with code {code} "
                            f"({'bad argument' if code == -1 else 'launch failure' if code == -2 else 'unknown'})")


def torch_ops():
    """Load (once) libhv_torch_ops.so and return the `torch.ops.hv` namespace; raises HVKernelError if it is not built."""
    global _hv
    if _hv is not None:
        return _hv
    import torch
    if not os.path.exists(TORCH_OPS_PATH):
        raise HVKernelError(
            f"{TORCH_OPS_PATH} is missing: the PyTorch custom-op library is not built (run __graft_entry__.build()). "
            "hunyuanvideo_efficiency_amd has no CPU or eager fallback.")
    torch.ops.load_library(TORCH_OPS_PATH)
    hv = torch.ops.hv
    v = int(hv.abi_version())
    if v != ABI_VERSION:
        raise HVKernelError(f"libhv_torch_ops / libhv_kernels ABI {v} != expected {ABI_VERSION}: rebuild the extension")
    for name in list(SIGNATURES) + list(CONTENT_SIGNATURES) + list(TEMPORAL_SIGNATURES) + list(GSSIM_SIGNATURES) + list(YUVW_SIGNATURES) + \
            list(MOTION_SIGNATURES) + list(MJPEG_SIGNATURES) + list(MJPEG_READ_SIGNATURES) + list(MJPEG_SYNC_SIGNATURES):
        if not hasattr(hv, name[len("hv_"):]):
            raise HVKernelError(f"{TORCH_OPS_PATH} does not register torch.ops.hv.{name[len('hv_'):]}")
    _hv = hv
    return hv


def call(name: str, *args):
    """torch.ops.hv.<name>(*args): tensors (or None), ints, floats, int lists - see the schema in csrc/hv_torch_ops.cpp.
    A non-zero kernel return code, a CPU tensor or a tensor on another GPU surfaces as HVKernelError."""
    op = getattr(torch_ops(), name)
    try:
        return op(*args)
    except (RuntimeError, NotImplementedError) as e:
        raise HVKernelError(f"hv::{name}: {str(e).splitlines()[0]}") from e


def host(name: str, *args) -> int:
    """Pure host queries of the ABI (no tensors): abi_version, attn_workspace_bytes, attn_suggest_splits."""
    return int(getattr(torch_ops(), name)(*args))
