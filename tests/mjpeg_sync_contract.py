"""The argument contract of include/hv_mjpeg_sync.h as a table, in the form of tests/mjpeg_read_contract.py (whose helpers and `call`
shape it keeps): the accepted baseline call of hv_mjpeg_decode_coefs_sync, the class of every pointer (iters alone may be NULL), every
refusal hv_mjpeg_decode_coefs states (the header takes them over) with an accepted neighbour, the two refusals of its own (sub_bytes
outside HV_MJPEG_SYNC_MIN_SUB .. HV_MJPEG_SYNC_MAX_SUB, iters not aligned to 4 bytes) and the last accepted value of every limit.
tests/test_mjpeg_sync_cpu.py drives it through ctypes on a machine without a GPU."""
import ctypes as C

from hunyuanvideo_efficiency_amd import _abi
from tests.abi_contract import ARG, I31, I63, LAUNCH, OK, PTR, Entry
from tests.mjpeg_read_contract import MAX_SIDE, PER_MCU, bits, coef_query, huff

M = _abi.MJPEG_SYNC_MACROS
MIN_SUB, MAX_SUB, LANES = M["HV_MJPEG_SYNC_MIN_SUB"], M["HV_MJPEG_SYNC_MAX_SUB"], M["HV_MJPEG_SYNC_LANES"]

E = {}

_DEC = dict(data=PTR + 8192, data_bytes=4096, interval_begin=PTR, interval_end=PTR + 64, T=1, H=16, W=32, Ri=1, ipf=2, huff_tables=huff(),
            sub_bytes=64, coefs=PTR + 1024, coef_bytes=2 * PER_MCU, status=PTR + 512, iters=PTR + 768)
E["hv_mjpeg_decode_coefs_sync"] = (
    Entry(_DEC, required=("data", "interval_begin", "interval_end", "huff_tables", "coefs", "status"), nullable=("iters",))
    .no("sub_bytes >= HV_MJPEG_SYNC_MIN_SUB", sub_bytes=MIN_SUB - 1).no("sub_bytes >= HV_MJPEG_SYNC_MIN_SUB", sub_bytes=0)
    .no("sub_bytes >= HV_MJPEG_SYNC_MIN_SUB", sub_bytes=-64).no("sub_bytes <= HV_MJPEG_SYNC_MAX_SUB", sub_bytes=MAX_SUB + 1)
    .yes("no power-of-two rule", sub_bytes=17)
    .no("iters aligned to int32", iters=PTR + 770).no("iters aligned to int32", iters=PTR + 769).yes("int32 needs 4 bytes", iters=PTR + 772)
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
    .yes("a table without codes", huff_tables=huff(dc=(bits(), [])))
    .limit("sub_bytes from HV_MJPEG_SYNC_MIN_SUB", dict(sub_bytes=MIN_SUB), dict(sub_bytes=MIN_SUB - 1))
    .limit("sub_bytes up to HV_MJPEG_SYNC_MAX_SUB", dict(sub_bytes=MAX_SUB), dict(sub_bytes=MAX_SUB + 1))
    .limit("code lengths exactly used up", dict(huff_tables=huff(dc=(bits(l1=2), [0, 1]))), dict(huff_tables=huff(dc=(bits(l1=2, l16=1), [0, 1, 2]))))
    .limit("DC symbols up to 11", dict(huff_tables=huff(dc=(bits(l2=2), [0, 11]), which=2)))
    .limit("AC sizes up to 10", dict(huff_tables=huff(ac=(bits(l2=2), [0x00, 0xFA]), which=1)))
    .limit("coef_bytes >= hv_mjpeg_coef_bytes", dict(coef_bytes=coef_query(1, 16, 32)), dict(coef_bytes=2 * PER_MCU - 1))
    .limit("W <= HV_YUV_MAX_SIDE", dict(W=MAX_SIDE, Ri=0, ipf=1, coef_bytes=coef_query(1, 16, MAX_SIDE)),
           dict(W=MAX_SIDE + 1, Ri=0, ipf=1, coef_bytes=I63))
    .limit("H <= HV_YUV_MAX_SIDE", dict(H=MAX_SIDE, Ri=0, ipf=1, coef_bytes=coef_query(1, MAX_SIDE, 32)),
           dict(H=MAX_SIDE + 1, Ri=0, ipf=1, coef_bytes=I63))
    .limit("T * ipf <= 2^31 - 1", dict(T=I31, Ri=0, ipf=1, coef_bytes=I63), dict(T=1 << 30, coef_bytes=I63)))


def stream_decls():
    """name -> [(C type, parameter)] of the declarations of hv_mjpeg_sync.h"""
    return {name: params for _, name, params in _abi.MJPEG_SYNC_DECLS}


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
