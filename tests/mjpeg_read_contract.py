"""The argument contract of include/hv_mjpeg_read.h as a table, in the form of tests/mjpeg_contract.py (whose `call` shape it keeps) and
tests/abi_contract.py (whose Entry class and constants it uses): one accepted baseline call per entry point, the class of every
pointer, one row per refusal the header states with an accepted neighbour, the last accepted value of every limit, the Huffman and
quantisation tables the entry points refuse (they are host arrays: real memory here), and the rules of the size query.
tests/test_mjpeg_read_refusals_cpu.py drives it through ctypes on a machine without a GPU."""
import ctypes as C

from hunyuanvideo_efficiency_amd import _abi
from tests import mjpeg_read_ref as R
from tests.abi_contract import ARG, I31, I63, LAUNCH, OK, PTR, Entry

M = _abi.MJPEG_READ_MACROS
MAX_SIDE = _abi.MACROS["HV_YUV_MAX_SIDE"]
PER_MCU = M["HV_MJPEG_COEF_BYTES_PER_MCU"]


def u8s(v):
    return (C.c_uint8 * len(v))(*v)


def huff(dc=None, ac=None, which=0):
    """the Annex K tables with table `which` (0, 2: DC; 1, 3: AC) replaced by (BITS, HUFFVAL)"""
    tabs = list(R.ANNEX_K)
    if dc is not None:
        tabs[which] = dc
    if ac is not None:
        tabs[which] = ac
    assert len(R.huff_bytes(tabs)) == M["HV_MJPEG_HUFF_BYTES"]
    return u8s(R.huff_bytes(tabs))


def bits(**at):
    """BITS with at['l<n>'] codes of length n"""
    b = [0] * 16
    for k, v in at.items():
        b[int(k[1:]) - 1] = v
    return b


def quant(**at):
    """all steps 16, entry at['q<i>'] of the 128 replaced"""
    q = [16] * M["HV_MJPEG_QUANT_BYTES"]
    for k, v in at.items():
        q[int(k[1:])] = v
    return u8s(q)


def coef_query(T, H, W):
    return lambda lib: lib.hv_mjpeg_coef_bytes(T, H, W)


E = {}

E["hv_mjpeg_find_restarts"] = (
    Entry(dict(data=PTR + 8192, data_bytes=4096, scan_begin=PTR, scan_end=PTR + 64, T=1, ipf=2, interval_begin=PTR + 128,
               interval_end=PTR + 256, found=PTR + 512),
          required=("data", "scan_begin", "scan_end", "interval_begin", "interval_end", "found"))
    .no("T >= 1", T=0).no("T >= 1", T=-1).no("ipf >= 1", ipf=0).no("ipf >= 1", ipf=-1).yes("one interval per frame", ipf=1)
    .no("data_bytes >= 0", data_bytes=-1).yes("no data at all", data_bytes=0).yes("data has no alignment rule", data=PTR + 8193)
    .no("scan_begin aligned to int64", scan_begin=PTR + 4).no("scan_end aligned to int64", scan_end=PTR + 68)
    .no("interval_begin aligned to int64", interval_begin=PTR + 129).no("interval_end aligned to int64", interval_end=PTR + 260)
    .yes("int64 needs 8 bytes", scan_begin=PTR + 8, scan_end=PTR + 72, interval_begin=PTR + 136, interval_end=PTR + 264)
    .no("found aligned to int32", found=PTR + 514).yes("int32 needs 4 bytes", found=PTR + 516)
    .limit("T * ipf <= 2^31 - 1", dict(T=I31, ipf=1), dict(T=1 << 30, ipf=2))
    .limit("T * ipf <= 2^31 - 1", dict(T=1, ipf=I31), dict(T=2, ipf=I31)))

_DEC = dict(data=PTR + 8192, data_bytes=4096, interval_begin=PTR, interval_end=PTR + 64, T=1, H=16, W=32, Ri=1, ipf=2, huff_tables=huff(),
            coefs=PTR + 1024, coef_bytes=2 * PER_MCU, status=PTR + 512)
E["hv_mjpeg_decode_coefs"] = (
    Entry(_DEC, required=("data", "interval_begin", "interval_end", "huff_tables", "coefs", "status"))
    .no("T >= 1", T=0).no("T >= 1", T=-1).no("data_bytes >= 0", data_bytes=-1).yes("no data at all", data_bytes=0)
    .no("W positive", W=0).no("H positive", H=0).no("W positive", W=-16).no("H positive", H=-16)
    .yes("no even-size rule", W=31, H=15).yes("the smallest frame", W=1, H=1, Ri=0, ipf=1)
    .no("Ri >= 0", Ri=-1).no("ipf = (mpf + Ri - 1) / Ri", ipf=1).no("ipf = (mpf + Ri - 1) / Ri", ipf=3).no("ipf = 1 for Ri = 0", Ri=0)
    .yes("one interval per frame", Ri=0, ipf=1).yes("an interval of the whole frame", Ri=2, ipf=1).yes("an interval longer than the frame", Ri=5, ipf=1)
    .yes("intervals across MCU rows", H=32, Ri=3, ipf=2, coef_bytes=4 * PER_MCU)
    .no("interval_begin aligned to int64", interval_begin=PTR + 4).no("interval_end aligned to int64", interval_end=PTR + 65)
    .yes("int64 needs 8 bytes", interval_begin=PTR + 8, interval_end=PTR + 72)
    .no("status aligned to int32", status=PTR + 514).yes("int32 needs 4 bytes", status=PTR + 516)
    .no("coefs aligned to 16 bytes", coefs=PTR + 1032).no("coefs aligned to 16 bytes", coefs=PTR + 1026).yes("16 bytes", coefs=PTR + 1040)
    .yes("data has no alignment rule", data=PTR + 8193).yes("a larger workspace", coef_bytes=2 * PER_MCU + 1)
    .no("over-subscribed code lengths", huff_tables=huff(dc=(bits(l1=3), [0, 1, 2])))
    .no("over-subscribed code lengths", huff_tables=huff(ac=(bits(l1=1, l2=2, l3=1), [1, 2, 3, 4]), which=3))
    .no("more than 256 symbols", huff_tables=huff(ac=(bits(l15=2, l16=255), [1] * 256), which=1))
    .no("a DC symbol above 11", huff_tables=huff(dc=(bits(l2=2), [0, 12]), which=2))
    .no("an AC size above 10", huff_tables=huff(ac=(bits(l2=2), [0x00, 0x0B]), which=1))
    .no("an AC size above 10", huff_tables=huff(ac=(bits(l2=2), [0x00, 0xFF]), which=3))
    .yes("a table without codes", huff_tables=huff(dc=(bits(), [])))
    .limit("code lengths exactly used up", dict(huff_tables=huff(dc=(bits(l1=2), [0, 1]))), dict(huff_tables=huff(dc=(bits(l1=2, l16=1), [0, 1, 2]))))
    .limit("256 symbols", dict(huff_tables=huff(ac=(bits(l15=1, l16=255), [1] * 256), which=1)))
    .limit("DC symbols up to 11", dict(huff_tables=huff(dc=(bits(l2=2), [0, 11]), which=2)))
    .limit("AC sizes up to 10", dict(huff_tables=huff(ac=(bits(l2=2), [0x00, 0xFA]), which=1)))
    .limit("coef_bytes >= hv_mjpeg_coef_bytes", dict(coef_bytes=coef_query(1, 16, 32)), dict(coef_bytes=2 * PER_MCU - 1))
    .limit("W <= HV_YUV_MAX_SIDE", dict(W=MAX_SIDE, Ri=0, ipf=1, coef_bytes=coef_query(1, 16, MAX_SIDE)),
           dict(W=MAX_SIDE + 1, Ri=0, ipf=1, coef_bytes=I63))
    .limit("H <= HV_YUV_MAX_SIDE", dict(H=MAX_SIDE, Ri=0, ipf=1, coef_bytes=coef_query(1, MAX_SIDE, 32)),
           dict(H=MAX_SIDE + 1, Ri=0, ipf=1, coef_bytes=I63))
    .limit("T * ipf <= 2^31 - 1", dict(T=I31, Ri=0, ipf=1, coef_bytes=I63), dict(T=1 << 30, coef_bytes=I63))
    .limit("both sides at HV_YUV_MAX_SIDE, an interval per MCU", dict(W=MAX_SIDE, H=MAX_SIDE, Ri=1, ipf=1 << 20, coef_bytes=I63)))

_CLIP = dict(coefs=PTR, coef_bytes=PER_MCU, quant_tables=quant(), vtab=PTR + 4096, out=PTR + 8192, dtype=0, sc=256, st=768, sh=16, T=1, H=16,
             W=16)
_WIDE = dict(W=80, sh=80, sc=1280, st=3840)
E["hv_mjpeg_coefs_to_clip"] = (
    Entry(_CLIP, required=("coefs", "quant_tables", "vtab", "out"))
    .no("dtype 0 | 1", dtype=2).no("dtype 0 | 1", dtype=-1).yes("fp32", dtype=1)
    .no("T >= 1", T=0).no("T >= 1", T=-1).no("W positive", W=0).no("H positive", H=0).no("W positive", W=-1).no("H positive", H=-1)
    .yes("no even-size rule", W=15, H=15).yes("the smallest frame", W=1, H=1)
    .no("a quantisation step of 0", quant_tables=quant(q0=0)).no("a quantisation step of 0", quant_tables=quant(q63=0))
    .no("a quantisation step of 0", quant_tables=quant(q64=0)).no("a quantisation step of 0", quant_tables=quant(q127=0))
    .yes("steps 1 and 255", quant_tables=quant(q0=1, q63=255, q64=255, q127=1))
    .no("coefs aligned to 16 bytes", coefs=PTR + 8).no("coefs aligned to 16 bytes", coefs=PTR + 2).yes("16 bytes", coefs=PTR + 16)
    .no("out aligned to fp16", out=PTR + 8193).yes("fp16 needs 2 bytes", out=PTR + 8194)
    .no("out aligned to fp32", dtype=1, out=PTR + 8194).yes("fp32 needs 4 bytes", dtype=1, out=PTR + 8196)
    .no("vtab aligned to fp16", vtab=PTR + 4097).yes("fp16 needs 2 bytes", vtab=PTR + 4098)
    .no("vtab aligned to fp32", dtype=1, vtab=PTR + 4098).yes("fp32 needs 4 bytes", dtype=1, vtab=PTR + 4100)
    .no("negative stride", sc=-256).no("negative stride", st=-768).no("negative stride", sh=-16)
    .no("rows overlap: sh < W", sh=15).no("channels overlap", sc=255).no("channels on one address", sc=0)
    .no("frames overlap", T=2, st=767, coef_bytes=2 * PER_MCU).no("frames on one address", T=2, st=0, coef_bytes=2 * PER_MCU)
    .yes("frames tight", T=2, st=768, coef_bytes=2 * PER_MCU).yes("one frame: st is free", st=0)
    .yes("a frame slice of a larger clip", T=2, st=256, sc=512, coef_bytes=2 * PER_MCU).yes("padded rows", sh=24, sc=24 * 16, st=3 * 24 * 16)
    .yes("a larger workspace", coef_bytes=PER_MCU + 1).yes("a wide frame", coef_bytes=5 * PER_MCU, **_WIDE)
    .limit("coef_bytes >= hv_mjpeg_coef_bytes", dict(coef_bytes=coef_query(1, 16, 16)), dict(coef_bytes=PER_MCU - 1))
    .limit("W <= HV_YUV_MAX_SIDE", dict(W=MAX_SIDE, sh=MAX_SIDE, sc=16 * MAX_SIDE, st=48 * MAX_SIDE, coef_bytes=coef_query(1, 16, MAX_SIDE)),
           dict(W=MAX_SIDE + 1, sh=MAX_SIDE + 1, sc=16 * (MAX_SIDE + 1), st=48 * (MAX_SIDE + 1), coef_bytes=I63))
    .limit("H <= HV_YUV_MAX_SIDE", dict(H=MAX_SIDE, sc=16 * MAX_SIDE, st=48 * MAX_SIDE, coef_bytes=coef_query(1, MAX_SIDE, 16)),
           dict(H=MAX_SIDE + 1, sc=16 * (MAX_SIDE + 1), st=48 * (MAX_SIDE + 1), coef_bytes=I63))
    .limit("tiles of 64 x 32 pixels fit grid.x", dict(T=I31, coef_bytes=I63), dict(T=I31, coef_bytes=I63, **_WIDE)))

# the size query: (T, H, W) -> bytes; 0 for refused shapes
QUERY = [((1, 1, 1), PER_MCU), ((1, 16, 16), PER_MCU), ((1, 17, 16), 2 * PER_MCU), ((1, 16, 17), 2 * PER_MCU), ((2, 17, 33), 2 * 2 * 3 * PER_MCU),
         ((129, 720, 1280), 129 * 45 * 80 * PER_MCU), ((I31, MAX_SIDE, MAX_SIDE), I31 * 1024 * 1024 * PER_MCU),
         ((0, 16, 16), 0), ((-1, 16, 16), 0), ((1, 0, 16), 0), ((1, 16, 0), 0), ((1, -16, 16), 0), ((1, MAX_SIDE + 1, 16), 0),
         ((1, 16, MAX_SIDE + 1), 0), ((1, MAX_SIDE, MAX_SIDE), 1024 * 1024 * PER_MCU)]


def stream_decls():
    """name -> [(C type, parameter)] of the declarations of hv_mjpeg_read.h that take a hipStream_t"""
    return {name: params for _, name, params in _abi.MJPEG_READ_DECLS if any(t == "hipStream_t" for t, _ in params)}


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
