"""The argument contract of include/hv_mjpeg.h as a table, in the form of tests/abi_contract.py (whose Entry class and constants it uses)
and tests/yuv_write_contract.py: one accepted baseline call per entry point, the class of every pointer, one row per refusal the header
states with an accepted neighbour, the last accepted value of every limit.  tests/test_mjpeg_refusals_cpu.py drives it through ctypes on a
machine without a GPU."""
import ctypes as C

from hunyuanvideo_efficiency_amd import _abi
from tests.abi_contract import ARG, LAUNCH, OK, PTR, Entry

M = _abi.MJPEG_MACROS
MAX_SIDE = _abi.MACROS["HV_YUV_MAX_SIDE"]

E = {}

_CLIP = dict(x=PTR, dtype=0, C=3, sc=64, st=192, sh=8, T=1, H=8, W=8, rescale=0, quality=90)


def _clip_rules(e):
    """the rules the two entry points share: everything about the clip and the quality"""
    return (e.no("dtype 0 | 1", dtype=2).no("dtype 0 | 1", dtype=-1).yes("fp32", dtype=1)
            .no("rescale 0 | 1", rescale=2).no("rescale 0 | 1", rescale=-1).yes("rescale = 1", rescale=1)
            .no("quality 1 .. 100", quality=0).no("quality 1 .. 100", quality=101).no("quality 1 .. 100", quality=-90)
            .yes("the lowest quality", quality=1).yes("the highest quality", quality=100)
            .no("C 1 | 3", C=0).no("C 1 | 3", C=2).no("C 1 | 3", C=4).no("C 1 | 3", C=-1).yes("gray", C=1)
            .no("T >= 1", T=0).no("T >= 1", T=-1).yes("many frames", T=1 << 20)
            .no("W positive", W=0).no("W positive", W=-2).no("H positive", H=0).no("H positive", H=-2)
            .yes("no even-size rule", W=7, H=7).yes("the smallest frame", W=1, H=1).yes("one pixel past an MCU", W=17, H=17)
            .no("negative stride", sc=-1).no("negative stride", st=-1).no("negative stride", sh=-1)
            .yes("the input is only read: an expanded view", sc=0, st=0, sh=0).yes("overlapping rows", sh=3)
            .yes("strides are free above 0", sc=1 << 40, st=1 << 41, sh=1 << 33)
            .no("x aligned to fp16", x=PTR + 1).yes("fp16 needs 2 bytes", x=PTR + 2)
            .no("x aligned to fp32", dtype=1, x=PTR + 2).no("x aligned to fp32", dtype=1, x=PTR + 1).yes("fp32 needs 4 bytes", dtype=1, x=PTR + 4)
            .limit("W <= HV_YUV_MAX_SIDE", dict(W=MAX_SIDE), dict(W=MAX_SIDE + 1))
            .limit("H <= HV_YUV_MAX_SIDE", dict(H=MAX_SIDE), dict(H=MAX_SIDE + 1))
            .limit("both sides at HV_YUV_MAX_SIDE, fp32, T at the int limit", dict(W=MAX_SIDE, H=MAX_SIDE, dtype=1, T=0x7FFFFFFF)))


E["hv_mjpeg_measure"] = (
    _clip_rules(Entry(dict(_CLIP, interval_bytes=PTR), required=("x", "interval_bytes")))
    .no("interval_bytes aligned to int32", interval_bytes=PTR + 1).no("interval_bytes aligned to int32", interval_bytes=PTR + 2)
    .yes("int32 needs 4 bytes", interval_bytes=PTR + 4))
E["hv_mjpeg_write"] = (
    _clip_rules(Entry(dict(_CLIP, offsets=PTR, scan=PTR + 4096), required=("x", "offsets", "scan")))
    .no("offsets aligned to int64", offsets=PTR + 4).no("offsets aligned to int64", offsets=PTR + 1).yes("int64 needs 8 bytes", offsets=PTR + 8)
    .yes("scan has no alignment rule", scan=PTR + 4097).yes("scan has no alignment rule", scan=PTR + 4100))


def stream_decls():
    """name -> [(C type, parameter)] of the declarations of hv_mjpeg.h that take a hipStream_t"""
    return {name: params for _, name, params in _abi.MJPEG_DECLS if any(t == "hipStream_t" for t, _ in params)}


def call(lib, name, overrides=None):
    """the entry point at its baseline with `overrides` applied, NULL stream -> return code"""
    vals = dict(E[name].base)
    unknown = set(overrides or ()) - set(vals)
    assert not unknown, f"{name}: overrides {sorted(unknown)} name no parameter of the baseline"
    vals.update(overrides or {})
    args = []
    for ctype, p in stream_decls()[name]:
        v = None if ctype == "hipStream_t" else vals[p]
        if callable(v):
            v = v(lib)
        if isinstance(v, C.Array):
            v = C.cast(v, C.c_void_p)
        args.append(v)
    return getattr(lib, name)(*args)


def rows():
    """every parametrised case: (id, entry point, overrides, expected code)"""
    out = []
    for name, e in E.items():
        out.append((f"{name}-baseline", name, {}, LAUNCH))
        for p in e.required:
            out.append((f"{name}-NULL-{p}", name, {p: None}, ARG))
        for kind, lst, want in (("refuse", e.refuse, ARG), ("accept", e.accept, LAUNCH), ("early", e.early, OK)):
            for i, (rule, ov) in enumerate(lst):
                out.append((f"{name}-{kind}{i}-{rule}", name, ov, want))
        for i, (rule, _, ok, bad) in enumerate(e.limits):
            out.append((f"{name}-limit{i}-ok-{rule}", name, ok, LAUNCH))
            if bad is not None:
                out.append((f"{name}-limit{i}-refuse-{rule}", name, bad, ARG))
    return out
