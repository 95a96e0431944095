#!/usr/bin/env python3
"""Generate hunyuanvideo_efficiency_amd/csrc/hv_torch_ops.cpp from include/hv_kernels.h.

Every `extern "C"` entry point of the C ABI becomes one PyTorch custom op `torch.ops.hv.<name without hv_>`
(TORCH_LIBRARY(hv, m) + TORCH_LIBRARY_IMPL(hv, CUDA, m); SURVEY.md 8b last row, BASELINE.json north_star "exposed to
Python through PyTorch-ROCm custom ops").  Mapping of the C parameters:
    const void* / const float* / const int* (device)  ->  Tensor?           (None = NULL)
    void* / float* (device, written)                 ->  Tensor(x!)?       (None = NULL)
    const int64_t* *_strides / const int* dims (host) ->  int[]
    int / int64_t -> int,  float -> float,  hipStream_t -> the current HIP stream of the tensors' device
Kernels return () and raise (TORCH_CHECK) on a non-zero C return code; the three pure host queries return int.
The entry points of include/hv_content.h go to csrc/hv_content_torch_ops.cpp the same way, as a TORCH_LIBRARY_FRAGMENT of `hv`, and
those of include/hv_temporal.h to csrc/hv_temporal_torch_ops.cpp, those of include/hv_gssim.h to csrc/hv_gssim_torch_ops.cpp, those of
include/hv_yuv_write.h to csrc/hv_yuv_write_torch_ops.cpp, those of include/hv_motion.h to csrc/hv_motion_torch_ops.cpp,
those of include/hv_mjpeg.h to csrc/hv_mjpeg_torch_ops.cpp, those of include/hv_mjpeg_read.h to csrc/hv_mjpeg_read_torch_ops.cpp (its two
host tables, const uint8_t* huff_tables / quant_tables, are int[] of the header's HV_MJPEG_HUFF_BYTES / HV_MJPEG_QUANT_BYTES entries 0 .. 255),
those of include/hv_mjpeg_sync.h to csrc/hv_mjpeg_sync_torch_ops.cpp.
Run:  python tools/gen_torch_ops.py            (rewrites the nine .cpp files; tests/test_capi_cpu.py, tests/test_content_refusals_cpu.py,
                                                tests/test_temporal_refusals_cpu.py, tests/test_gssim_refusals_cpu.py,
                                                tests/test_yuv_write_refusals_cpu.py, tests/test_motion_refusals_cpu.py and
                                                tests/test_mjpeg_refusals_cpu.py, tests/test_mjpeg_read_refusals_cpu.py and
                                                tests/test_mjpeg_sync_cpu.py check they are up to date)
      python tools/gen_torch_ops.py --record-abi    (after a bump of HV_ABI_VERSION: writes tests/golden/abi_v<N>.json, the
                                                      declarations the same test holds the header to until the next bump)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hunyuanvideo_efficiency_amd import _abi  # noqa: E402  (the one parser of include/hv_kernels.h)

OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_torch_ops.cpp")
CONTENT_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_content_torch_ops.cpp")   # from include/hv_content.h
TEMPORAL_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_temporal_torch_ops.cpp")   # from include/hv_temporal.h
GSSIM_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_gssim_torch_ops.cpp")   # from include/hv_gssim.h
YUVW_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_yuv_write_torch_ops.cpp")   # from include/hv_yuv_write.h
MOTION_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_motion_torch_ops.cpp")   # from include/hv_motion.h
MJPEG_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_torch_ops.cpp")   # from include/hv_mjpeg.h
MJPEG_READ_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_read_torch_ops.cpp")   # from include/hv_mjpeg_read.h
MJPEG_SYNC_OUT = os.path.join(ROOT, "hunyuanvideo_efficiency_amd", "csrc", "hv_mjpeg_sync_torch_ops.cpp")   # from include/hv_mjpeg_sync.h
HOST_BYTES = {"huff_tables": _abi.MJPEG_READ_MACROS["HV_MJPEG_HUFF_BYTES"], "quant_tables": _abi.MJPEG_READ_MACROS["HV_MJPEG_QUANT_BYTES"]}
HOST_ARRAYS = {"a_strides", "b_strides", "src_strides", "dst_strides", "dims"}
HOST_ARRAY_LEN = 4      # every host array of the C ABI is a 4-vector (hv_vae_blend_f16, hv_copy4d_16b: strides / dims of a 4-D view)


def classify(ctype, pname):
    c = ctype.replace(" ", "")
    if c == "hipStream_t":
        return "stream"
    if pname in HOST_BYTES:
        return "host_u8"
    if pname in HOST_ARRAYS:
        return "host_i64" if "int64_t" in c else "host_i32"
    if c.endswith("*"):
        return "tensor_in" if c.startswith("const") else "tensor_out"
    if c in ("int", "int64_t"):
        return "int"
    if c == "float":
        return "float"
    raise ValueError(f"unmapped C type {ctype!r} ({pname})")


def gen(decls=None, header="hv_kernels.h"):
    """the registration source for the declarations of `header`: the main header defines the `hv` library, any other header adds to it
    (TORCH_LIBRARY_FRAGMENT; both sources are linked into libhv_torch_ops.so)"""
    main = decls is None
    decls = _abi.DECLS if main else decls
    L = []
    A = L.append
    A(f"// GENERATED by tools/gen_torch_ops.py from include/{header} - do not edit by hand.")
    A("// PyTorch custom-op registration of the C ABI: torch.ops.hv.<op>(tensors, sizes...) -> launches the gfx950 kernel on the")
    A("// current HIP stream of the tensors' device.  There is no CPU implementation: a CPU tensor fails in the dispatcher.")
    A("#include <torch/library.h>")
    A("#include <ATen/core/Tensor.h>")
    A("#include <c10/hip/HIPStream.h>")
    A("#include <c10/hip/HIPGuard.h>")
    A("#include <optional>")
    A("#include <vector>")
    A(f'#include "../../include/{header}"')
    A("")
    A("namespace {")
    A("using OptT = std::optional<at::Tensor>;")
    A("")
    A("// device pointer of an optional tensor; records the device every present tensor must share")
    A("struct Dev {")
    A("    c10::DeviceIndex idx = -1;")
    A("    const char* op;")
    A("    explicit Dev(const char* o) : op(o) {}")
    A("    void* p(const OptT& t, const char* name) {")
    A("        if (!t.has_value() || !t->defined()) return nullptr;")
    A('        TORCH_CHECK(t->is_cuda(), "hv::", op, ": ", name, " must be a GPU tensor (this library has no CPU path), got ", t->device());')
    A("        if (idx < 0) idx = t->device().index();")
    A('        TORCH_CHECK(t->device().index() == idx, "hv::", op, ": ", name, " is on a different GPU than the other tensors");')
    A("        return t->data_ptr();")
    A("    }")
    A("};")
    A("")
    A("inline void check_rc(int rc, const char* op) {")
    A('    TORCH_CHECK(rc == 0, "hv::", op, " failed with code ", rc, rc == -1 ? " (bad argument)" : rc == -2 ? " (launch failure)" : "");')
    A("}")
    A("")
    schemas, impls_cuda, impls_host = [], [], []
    for ret, name, params in decls:
        op = name[len("hv_"):]
        kinds = [(classify(t, n), t, n) for t, n in params]
        has_stream = any(k == "stream" for k, _, _ in kinds)
        # schema
        sch, sig, pre, call = [], [], [], []
        alias = iter("abcdefgh")
        for k, t, n in kinds:
            if k == "stream":
                call.append("stream")
            elif k == "tensor_in":
                sch.append(f"Tensor? {n}")
                sig.append(f"const OptT& {n}")
                ct = t.replace(" ", "")
                call.append(f"({t})dev.p({n}, \"{n}\")")
            elif k == "tensor_out":
                sch.append(f"Tensor({next(alias)}!)? {n}")
                sig.append(f"const OptT& {n}")
                call.append(f"({t})dev.p({n}, \"{n}\")")
            elif k == "host_i64":
                sch.append(f"int[] {n}")
                sig.append(f"at::IntArrayRef {n}")
                pre.append(f'    TORCH_CHECK({n}.size() == {HOST_ARRAY_LEN}, "hv::{op}: {n} must have {HOST_ARRAY_LEN} elements, got ", {n}.size());')
                call.append(f"{n}.data()")
            elif k == "host_i32":
                sch.append(f"int[] {n}")
                sig.append(f"at::IntArrayRef {n}")
                pre.append(f'    TORCH_CHECK({n}.size() == {HOST_ARRAY_LEN}, "hv::{op}: {n} must have {HOST_ARRAY_LEN} elements, got ", {n}.size());')
                pre.append(f"    std::vector<int> {n}_i({n}.begin(), {n}.end());")
                call.append(f"{n}_i.data()")
            elif k == "host_u8":
                sch.append(f"int[] {n}")
                sig.append(f"at::IntArrayRef {n}")
                pre.append(f'    TORCH_CHECK({n}.size() == {HOST_BYTES[n]}, "hv::{op}: {n} must have {HOST_BYTES[n]} elements, got ", {n}.size());')
                pre.append(f'    for (auto v : {n}) TORCH_CHECK(v >= 0 && v <= 255, "hv::{op}: {n} holds bytes, got ", v);')
                pre.append(f"    std::vector<uint8_t> {n}_b({n}.begin(), {n}.end());")
                call.append(f"{n}_b.data()")
            elif k == "int":
                sch.append(f"int {n}")
                sig.append(f"int64_t {n}")
                call.append(f"({t}){n}")
            elif k == "float":
                sch.append(f"float {n}")
                sig.append(f"double {n}")
                call.append(f"(float){n}")
        if has_stream:
            schemas.append(f'    m.def("{op}({", ".join(sch)}) -> ()");')
            A(f"void op_{op}({', '.join(sig)}) {{")
            A(f'    Dev dev("{op}");')
            for ln in pre:
                A(ln)
            # evaluate pointers first (fixes the device), then guard + stream
            ptr_args = [c for c in call]
            A("    // pointers first: they fix the device whose current stream the kernel is enqueued on")
            tmp_names = []
            for i, c in enumerate(ptr_args):
                if "dev.p(" in c:
                    A(f"    auto a{i} = {c};")
                    tmp_names.append(f"a{i}")
                else:
                    tmp_names.append(c)
            A(f'    TORCH_CHECK(dev.idx >= 0, "hv::{op}: needs at least one GPU tensor");')
            A("    c10::hip::HIPGuard guard(dev.idx);")
            A("    hipStream_t stream = c10::hip::getCurrentHIPStream(dev.idx).stream();")
            A(f"    check_rc({name}({', '.join(tmp_names)}), \"{op}\");")
            A("}")
            A("")
            impls_cuda.append(f'    m.impl("{op}", &op_{op});')
        else:
            schemas.append(f'    m.def("{op}({", ".join(sch)}) -> int");')
            A(f"int64_t op_{op}({', '.join(sig)}) {{")
            A(f"    return (int64_t){name}({', '.join(call)});")
            A("}")
            A("")
            impls_host.append(f'    m.impl("{op}", &op_{op});')
    A("}  // namespace")
    A("")
    A("TORCH_LIBRARY(hv, m) {" if main else "TORCH_LIBRARY_FRAGMENT(hv, m) {")
    L.extend(schemas)
    A("}")
    A("")
    A("TORCH_LIBRARY_IMPL(hv, CUDA, m) {      // PyTorch-ROCm: HIP devices carry the CUDA dispatch key")
    L.extend(impls_cuda)
    A("}")
    A("")
    A("TORCH_LIBRARY_IMPL(hv, CompositeExplicitAutograd, m) {   // pure host queries (no tensor arguments)")
    L.extend(impls_host)
    A("}")
    return "\n".join(L) + "\n"


def record_abi():
    version = _abi.MACROS["HV_ABI_VERSION"]
    path = os.path.join(ROOT, "tests", "golden", f"abi_v{version}.json")
    decls = [{"name": name, "returns": ret, "params": [t for t, _ in params]} for ret, name, params in _abi.DECLS]
    with open(path, "w") as f:
        json.dump({"abi_version": version, "declarations": decls}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {len(decls)} declarations")


if __name__ == "__main__":
    if sys.argv[1:] == ["--record-abi"]:
        record_abi()
        sys.exit(0)
    for path, text in ((OUT, gen()), (CONTENT_OUT, gen(_abi.CONTENT_DECLS, "hv_content.h")),
                       (TEMPORAL_OUT, gen(_abi.TEMPORAL_DECLS, "hv_temporal.h")), (GSSIM_OUT, gen(_abi.GSSIM_DECLS, "hv_gssim.h")),
                       (YUVW_OUT, gen(_abi.YUVW_DECLS, "hv_yuv_write.h")), (MOTION_OUT, gen(_abi.MOTION_DECLS, "hv_motion.h")),
                       (MJPEG_OUT, gen(_abi.MJPEG_DECLS, "hv_mjpeg.h")), (MJPEG_READ_OUT, gen(_abi.MJPEG_READ_DECLS, "hv_mjpeg_read.h")),
                       (MJPEG_SYNC_OUT, gen(_abi.MJPEG_SYNC_DECLS, "hv_mjpeg_sync.h"))):
        with open(path, "w") as f:
            f.write(text)
        print(f"wrote {path}: {text.count('m.def(')} ops")
