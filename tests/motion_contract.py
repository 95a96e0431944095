"""The argument contract of include/hv_motion.h as a table, in the form of tests/abi_contract.py (whose Entry class and constants it
uses): one accepted baseline call, the class of every pointer, one row per refusal the header states, the last accepted value of every
limit, the early-out.  tests/test_motion_refusals_cpu.py drives it through ctypes on a machine without a GPU."""
import ctypes as C

from hunyuanvideo_efficiency_amd import _abi
from tests.abi_contract import ARG, LAUNCH, OK, PTR, Entry

M = _abi.MOTION_MACROS
_MAXR, _MAXLAM = M["HV_MOTION_MAX_RADIUS"], M["HV_MOTION_MAX_LAM"]

E = {}

_MOTION = dict(x=PTR, sc=1, st=1, sh=1, dtype=0, T=2, H=1, W=1, rescale=0, wr=1, wg=0, wb=0, round=0, shift=0, block=16, radius=1, lam=0,
               mv=PTR, sad=PTR, sad0=PTR)
E["hv_block_motion"] = (
    Entry(_MOTION, required=("x", "mv", "sad", "sad0"))
    .out("T == 1: no pairs, nothing enqueued", T=1)
    .out("T == 1: the outputs may be NULL", T=1, mv=None, sad=None, sad0=None)
    .no("T == 1 still needs x", T=1, x=None).no("T == 1 still checks the parameters", T=1, block=4)
    .no("dtype 0 | 1", dtype=2).no("dtype 0 | 1", dtype=-1).yes("fp32", dtype=1).no("rescale 0 | 1", rescale=2).yes("rescale = 1", rescale=1)
    .no("T >= 1", T=0).no("H >= 1", H=0).no("W >= 1", W=0)
    .no("overlapping strides: sh >= W", sh=0).no("negative stride", sc=-1).no("negative stride", st=-1)
    .yes("channel and frame strides may be 0 (overlapping reads)", sc=0, st=0)
    .no("weights >= 0", wr=-1).no("weights >= 0", wg=-1).no("weights >= 0", wb=-1).no("round >= 0", round=-1).no("shift >= 0", shift=-1)
    .no("the luma stays a byte", wr=2).no("the luma stays a byte", round=1).no("weights <= 2^22", wr=(1 << 22) + 1, shift=22)
    .limit("shift <= 22", dict(wr=1 << 22, shift=22), dict(wr=1 << 22, shift=23))
    .no("block 8 | 16", block=0).no("block 8 | 16", block=4).no("block 8 | 16", block=12).no("block 8 | 16", block=32).yes("block = 8", block=8)
    .no("radius >= 1", radius=0).no("radius >= 1", radius=-1).no("lam >= 0", lam=-1)
    .limit("radius <= HV_MOTION_MAX_RADIUS", dict(radius=_MAXR), dict(radius=_MAXR + 1), macros=("HV_MOTION_MAX_RADIUS",))
    .limit("lam <= HV_MOTION_MAX_LAM", dict(lam=_MAXLAM), dict(lam=_MAXLAM + 1), macros=("HV_MOTION_MAX_LAM",))
    .no("mv 4-byte aligned", mv=PTR + 2).no("sad 4-byte aligned", sad=PTR + 2).no("sad0 4-byte aligned", sad0=PTR + 2)
    .no("alignment is checked for T == 1 too", T=1, mv=PTR + 2)
    .limit("T <= 65535", dict(T=65535), dict(T=65536))
    .limit("H <= 65536", dict(H=65536), dict(H=65537))
    .limit("W <= 65536", dict(W=65536, sh=65536), dict(W=65537, sh=65537))
    .limit("H * W <= 2^31 - 1", dict(H=65536, W=32767, sh=32767), dict(H=65536, W=32768, sh=32768))
    .limit("a workgroup per HV_MOTION_TILE x HV_MOTION_TILE pixels: any H, W", dict(H=M["HV_MOTION_TILE"] + 1, W=M["HV_MOTION_TILE"] + 1,
                                                                                   sh=M["HV_MOTION_TILE"] + 1), macros=("HV_MOTION_TILE",)))


def stream_decls():
    """name -> [(C type, parameter)] of the declarations of hv_motion.h that take a hipStream_t"""
    return {name: params for _, name, params in _abi.MOTION_DECLS if any(t == "hipStream_t" for t, _ in params)}


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
