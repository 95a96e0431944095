"""The argument contract of include/hv_content.h as a table, in the form of tests/abi_contract.py (whose Entry class and constants it
uses): one accepted baseline call per stream entry point, the class of every pointer, one row per refusal the header states, the last
accepted value of every limit, the early-outs; the shapes the host query answers with 0 and the size rule that ties it to its kernel.
tests/test_content_refusals_cpu.py drives it through ctypes on a machine without a GPU."""
import ctypes as C

from hunyuanvideo_efficiency_amd import _abi
from tests.abi_contract import ARG, I31, I63, LAUNCH, OK, PTR, Entry

M = _abi.CONTENT_MACROS
_CHUNK, _IBINS = M["HV_CONTENT_CHUNK"], M["HV_CONTENT_INTER_BINS"]
_ROW2 = (2 * 256 + _IBINS) * 4          # bytes of one chunk's partial rows for T = 2

E = {}


def _content_ws(*a):
    return lambda lib: lib.hv_content_histograms_workspace_bytes(*a)


_CONTENT = dict(x=PTR, sc=1, st=1, sh=1, dtype=0, T=2, H=1, W=1, rescale=0, wr=1, wg=0, wb=0, round=0, shift=0, intra=PTR, inter=PTR,
                workspace=PTR, workspace_bytes=_content_ws(2, 1, 1))
E["hv_content_histograms"] = (
    Entry(_CONTENT, required=("x", "intra", "inter", "workspace"))
    .yes("T == 1: no inter rows, inter may be NULL", T=1, inter=None, workspace_bytes=_content_ws(1, 1, 1))
    .no("dtype 0 | 1", dtype=2).no("dtype 0 | 1", dtype=-1).yes("fp32", dtype=1).no("rescale 0 | 1", rescale=2).yes("rescale = 1", rescale=1)
    .no("T >= 1", T=0).no("H >= 1", H=0).no("W >= 1", W=0)
    .no("overlapping strides: sh >= W", sh=0).no("negative stride", sc=-1).no("negative stride", st=-1)
    .yes("channel and frame strides may be 0 (overlapping reads)", sc=0, st=0)
    .no("weights >= 0", wr=-1).no("weights >= 0", wg=-1).no("weights >= 0", wb=-1).no("round >= 0", round=-1).no("shift >= 0", shift=-1)
    .no("the luma stays a byte", wr=2).no("the luma stays a byte", round=1).no("weights <= 2^22", wr=(1 << 22) + 1, shift=22)
    .limit("shift <= 22", dict(wr=1 << 22, shift=22), dict(wr=1 << 22, shift=23))
    .no("intra 4-byte aligned", intra=PTR + 2).no("inter 4-byte aligned", inter=PTR + 2).no("workspace 4-byte aligned", workspace=PTR + 2)
    .limit("T <= 65535", dict(T=65535, workspace_bytes=_content_ws(65535, 1, 1)), dict(T=65536, workspace_bytes=I63))
    .limit("H <= 65536", dict(H=65536, workspace_bytes=_content_ws(2, 65536, 1)), dict(H=65537, workspace_bytes=I63))
    .limit("W <= 65536", dict(W=65536, sh=65536, workspace_bytes=_content_ws(2, 1, 65536)), dict(W=65537, sh=65537, workspace_bytes=I63))
    .limit("H * W <= 2^31 - 1", dict(H=65536, W=32767, sh=32767, workspace_bytes=_content_ws(2, 65536, 32767)),
           dict(H=65536, W=32768, sh=32768, workspace_bytes=I63))
    .limit("workspace_bytes >= hv_content_histograms_workspace_bytes(T, H, W)", dict(),
           dict(workspace_bytes=lambda lib: lib.hv_content_histograms_workspace_bytes(2, 1, 1) - 1))
    .limit("workspace_bytes: one chunk of partial rows up to H * W = HV_CONTENT_CHUNK, (256 + HV_CONTENT_INTER_BINS) words for T = 2",
           dict(W=_CHUNK, sh=_CHUNK, workspace_bytes=_ROW2), dict(W=_CHUNK, sh=_CHUNK, workspace_bytes=_ROW2 - 1),
           macros=("HV_CONTENT_CHUNK", "HV_CONTENT_INTER_BINS"))
    .limit("workspace_bytes: a second chunk from H * W = HV_CONTENT_CHUNK + 1 on", dict(W=_CHUNK + 1, sh=_CHUNK + 1, workspace_bytes=2 * _ROW2),
           dict(W=_CHUNK + 1, sh=_CHUNK + 1, workspace_bytes=2 * _ROW2 - 1), macros=("HV_CONTENT_CHUNK",)))

E["hv_histogram_entropy"] = (
    Entry(dict(counts=PTR, rows=1, bins=256, origin=0, out=PTR), required=("counts", "out"))
    .no("rows >= 0", rows=-1).no("bins >= 1", bins=0).no("origin >= 0", origin=-1).no("origin <= bins", origin=257)
    .yes("origin == bins", origin=256).yes("a row of inter-frame differences", bins=_IBINS, origin=255)
    .no("counts 4-byte aligned", counts=PTR + 2).no("out 8-byte aligned", out=PTR + 4)
    .limit("bins <= 1024", dict(bins=1024), dict(bins=1025))
    .limit("rows <= 2^31 - 1", dict(rows=I31), dict(rows=I31 + 1))
    .out("rows == 0", rows=0))

QUERIES = {
    "hv_content_histograms_workspace_bytes": [((1, 1, 1), 256 * 4), ((2, 1, 1), _ROW2), ((2, 1, _CHUNK), _ROW2), ((2, 1, _CHUNK + 1), 2 * _ROW2),
                                              ((65535, 65536, 32767), None), ((0, 8, 8), 0), ((65536, 8, 8), 0), ((2, 0, 8), 0), ((2, 8, 0), 0),
                                              ((2, 65537, 8), 0), ((2, 8, 65537), 0), ((2, 65536, 32768), 0), ((-1, 8, 8), 0)],
}
SIZE_RULES = [("hv_content_histograms_workspace_bytes", (2, 1, 1), "hv_content_histograms", "workspace_bytes", 1)]


def stream_decls():
    """name -> [(C type, parameter)] of the declarations of hv_content.h that take a hipStream_t"""
    return {name: params for _, name, params in _abi.CONTENT_DECLS if any(t == "hipStream_t" for t, _ in params)}


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
        for p in e.nullable:
            out.append((f"{name}-NULL-ok-{p}", name, {p: None}, LAUNCH))
        for kind, lst, want in (("refuse", e.refuse, ARG), ("accept", e.accept, LAUNCH), ("early", e.early, OK)):
            for i, (rule, ov) in enumerate(lst):
                out.append((f"{name}-{kind}{i}-{rule}", name, ov, want))
        for i, (rule, _, ok, bad) in enumerate(e.limits):
            out.append((f"{name}-limit{i}-ok-{rule}", name, ok, LAUNCH))
            if bad is not None:
                out.append((f"{name}-limit{i}-refuse-{rule}", name, bad, ARG))
    return out
