"""TEST INFRASTRUCTURE: one call made on two implementations of a kernel entry point - the HIP wrapper and its CPU double
(tests/cpu_kernel_doubles.py), or a pristine double and a mutated copy - with everything a caller can observe compared.

compare_call(real_fn, double_fn, case) builds the case once per side (operands in NaN-poisoned memory, outputs in sentinel-filled
buffers: tests/guarded_memory.py), makes the call and applies, in this order, the checks whose names a ParityError carries:

  written-set       the cells of every watched buffer (operands, outputs, their pads and guard rows) whose bits changed are the same
                    cells on both sides
  return-structure  tensor / tuple / None, the same length, the same Python scalars (T, H, W; T * s)
  return-identity   a given out / out_q / out_scale (or the in-place operand) is the object returned, on both sides
  return-layout     the same shape and dtype; the same strides where the callee allocated the tensor
  values            class "copy" and "exact": the returned tensors, the derived values and every watched buffer bit for bit
  bounded           class "bounded": both sides pass the check function of the kernel's own edge test (no kernel-versus-double tolerance)

Value classes:
  copy     data movement or one correctly rounded conversion: bit-equal on arbitrary data (NaN payloads, signed zeros, infinities)
  exact    small integers and powers of two: every product and partial sum is exact in fp32 (|sum| < 2^24), so each documented rounding
           point rounds the same value in any summation order (certified on the CPU: tests/test_kernel_doubles_cpu.py)
  bounded  a transcendental function or a normalisation: the fp64 reference and bound of rowwise_bounds / error_bounds / conv_bounds /
           attention_bounds / the GroupNorm check of test_gpu_groupnorm_conditioning, applied to each side on its own

CASES is the one table of both tiers; REFUSALS the one table of illegal calls (each must raise on both sides and write nothing)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Optional

import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from oracle import dit_ref as R
from tests import activation_bounds as ACT
from tests import attention_bounds as AB
from tests import conv_bounds as CB
from tests import cpu_kernel_doubles as KD
from tests import error_bounds as EB
from tests import rowwise_bounds as RB
from tests.guarded_memory import INT, NAN_BITS, SENT, Guarded, GuardedBytes, GuardedFlat, Poisoned, crop, poisoned_vec

BF16, F16, F32, FP8, I32 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn, torch.int32
E = R.Prec(True)

# differences between a double and its kernel that are wanted (tests/test_kernel_doubles_cpu.py shows each is still real)
DELIBERATE_DEVIATIONS = {
    "sp.attn_suggest_splits": "returns 2 from 128 keys on, whatever n_q and the head count, to exercise both slot counts of the ring on the "
                              "small shapes of the CPU tier; the kernel's rule (hv_attn_suggest_splits) splits only where the grid is short",
    "ops.attn_fwd:unrounded-q": "the attention doubles multiply fp32(q) by the scale without the kernel's rounding of q' = bf16(q * scale * "
                                "log2 e): they follow the oracle's rounding points and are held to the bound of that contract "
                                "(attention_bounds.AttnRef(rounded_q=False)), as the sequence-parallel tests document",
    "ops.attn_fwd:narrow-view": "the attention doubles assert that q, k, v and out have at least n_heads * 128 columns; ops.attn_fwd asserts "
                                "nothing of the kind and hands the row stride to the kernel, which would read the next row's columns: the "
                                "double is stricter on purpose, so that such a view fails on the CPU tier",
}
# public wrappers that reach a kernel (call _lib.call) and have no double, with the reason
NO_DOUBLE = {
    "ops.euler_step_f32_": "the fp32-velocity form of the Euler step: only the batch sampler's fp32 CFG mix calls it, no CPU-tier test runs it",
    "vae_ops.blend_": "tile blending runs in tests/test_vae_tiling_cpu.py through its own torch reference of the tiling plan, not a double",
    "vae_ops.postprocess": "the final fp16 -> fp32 image map is outside the tile coder the CPU tier drives",
}


class ParityError(AssertionError):
    def __init__(self, check: str, what: str):
        super().__init__(f"[{check}] {what}")
        self.check = check


@dataclass
class Call:
    args: tuple
    kwargs: Dict[str, Any] = field(default_factory=dict)
    watch: Dict[str, torch.Tensor] = field(default_factory=dict)     # name -> a whole buffer (operand or output with its guard cells)
    same: Dict[int, torch.Tensor] = field(default_factory=dict)      # position in the flattened return -> the tensor it must BE
    ref: Any = None                                                  # what the bounded check needs (CPU tensors)
    post: Optional[Callable] = None                                  # (ret, call, peer) -> {name: tensor}: derived values, compared as returns


@dataclass
class Case:
    op: str                      # "ops.gemm", "vae_ops.conv_cout4", "sp.copy3d"
    name: str
    cls: str                     # copy | exact | bounded
    build: Callable              # (device, flip=False) -> Call; flip reverses the K / channel order of an exact case
    check: Optional[Callable] = None        # bounded: (call, flat, derived, peer, is_double) -> error-to-bound ratio; raises AssertionError
    flippable: bool = False
    any_nan: bool = False        # a CONVERSION to bf16 (not a bit copy): a NaN stays a NaN in the same cell, its sign and payload are free

    @property
    def id(self):
        return f"{self.op}:{self.name}"


# ------------------------------------------------------------------------------------------------------------ the two sides
def real_fn(op: str):
    space, name = op.split(".")
    if space == "sp":
        from hunyuanvideo_efficiency_amd.long_ctx_attention import _HipKernels
        return getattr(_HipKernels, name)
    import importlib
    return getattr(importlib.import_module("hunyuanvideo_efficiency_amd." + space), name)


def double_fn(op: str):
    space, name = op.split(".")
    if space == "sp":
        from tests.test_ulysses_gloo import CpuKernelDouble
        return getattr(CpuKernelDouble, name)
    if space == "vae_ops":
        return getattr(KD, KD.VAE_TILE_CODER_NAMES[name])
    return getattr(KD, name)


def real_peer(op):
    return real_fn(op)


def double_peer(op):
    return double_fn(op)


# ------------------------------------------------------------------------------------------------------------ comparison
def bits(t):
    t = t.detach()
    if t.dtype in (torch.int16, torch.int32, torch.uint8, torch.int64):
        return t.cpu().clone()
    return t.contiguous().view(INT[t.element_size()]).cpu().clone()


def canonical_nan16(b):
    """16-bit cells read as bf16: every NaN pattern (exponent all ones, mantissa not zero) becomes 0x7FC0"""
    if b.dtype != torch.int16:
        return b
    return torch.where((b & 0x7FFF) > 0x7F80, torch.full_like(b, 0x7FC0), b)


def _flatten(ret):
    if ret is None:
        return []
    if isinstance(ret, torch.Tensor):
        return [ret]
    if isinstance(ret, (tuple, list)):
        return [x for r in ret for x in _flatten(r)]
    if isinstance(ret, (int, float, bool)):
        return [ret]
    if hasattr(ret, "o") and hasattr(ret, "ml"):               # AttnPartials: compared attribute by attribute (see `post`)
        return [("AttnPartials",)]
    if hasattr(ret, "partial") and hasattr(ret, "M"):          # GNStats: the partial rows differ in layout by design (see `post`)
        return [("GNStats", int(ret.M), int(ret.C))]
    raise TypeError(f"unexpected return value {type(ret)}")


def _kind_of(ret):
    if isinstance(ret, (tuple, list)):
        return tuple(_kind_of(r) for r in ret)
    return "tensor" if isinstance(ret, torch.Tensor) else type(ret).__name__


@dataclass
class Side:
    call: Call
    before: Dict[str, torch.Tensor]
    after: Dict[str, torch.Tensor]
    ret: Any
    flat: list
    derived: Dict[str, torch.Tensor]


def run_side(fn, case: Case, device, peer, flip=False) -> Side:
    call = case.build(device, flip) if case.flippable else case.build(device)
    before = {k: bits(v) for k, v in call.watch.items()}
    ret = fn(*call.args, **call.kwargs)
    if str(device) != "cpu":
        torch.cuda.synchronize()
    after = {k: bits(v) for k, v in call.watch.items()}
    derived = call.post(ret, call, peer) if call.post is not None else {}
    return Side(call, before, after, ret, _flatten(ret), derived)


def compare_call(real, double, case: Case, real_device="cuda", double_device="cpu", real_peer_fn=real_peer, double_peer_fn=double_peer,
                 real_is_double=False):
    """returns the error-to-bound ratios (kernel, double) of a bounded case, (0.0, 0.0) otherwise; raises ParityError"""
    a = run_side(real, case, real_device, real_peer_fn)
    b = run_side(double, case, double_device, double_peer_fn)
    what = case.id
    # written set
    assert a.before.keys() == b.before.keys()
    for k in a.before:
        wa, wb = a.before[k] != a.after[k], b.before[k] != b.after[k]
        if not torch.equal(wa, wb):
            d = (wa != wb).nonzero()
            raise ParityError("written-set", f"{what}: buffer {k!r}: {d.shape[0]} cells written by one side only ({int((wa & ~wb).sum())} by the "
                                             f"kernel alone, {int((wb & ~wa).sum())} by the double alone), first at {d[0].tolist()}")
    # return value: structure, identity, layout
    if _kind_of(a.ret) != _kind_of(b.ret) or len(a.flat) != len(b.flat):
        raise ParityError("return-structure", f"{what}: kernel returns {_kind_of(a.ret)}, double {_kind_of(b.ret)}")
    for i, (x, y) in enumerate(zip(a.flat, b.flat)):
        if not isinstance(x, torch.Tensor) and x != y:
            raise ParityError("return-structure", f"{what}: return element {i}: kernel {x!r}, double {y!r}")
    for side, nm in ((a, "kernel"), (b, "double")):
        for i, t in side.call.same.items():
            if i >= len(side.flat) or side.flat[i] is not t:
                raise ParityError("return-identity", f"{what}: the {nm} does not return the tensor it was given (return element {i})")
    for i, (x, y) in enumerate(zip(a.flat, b.flat)):
        if isinstance(x, torch.Tensor):
            if tuple(x.shape) != tuple(y.shape) or x.dtype != y.dtype:
                raise ParityError("return-layout", f"{what}: return element {i}: kernel {tuple(x.shape)} {x.dtype}, double {tuple(y.shape)} {y.dtype}")
            if i not in a.call.same and x.stride() != y.stride():
                raise ParityError("return-layout", f"{what}: return element {i}: strides {x.stride()} (kernel) vs {y.stride()} (double)")
    if a.derived.keys() != b.derived.keys():
        raise ParityError("return-structure", f"{what}: derived values {sorted(a.derived)} vs {sorted(b.derived)}")
    # values
    if case.cls in ("copy", "exact"):
        pairs = [(f"buffer {k!r}", a.after[k], b.after[k]) for k in a.after]
        pairs += [(f"return element {i}", bits(x), bits(y)) for i, (x, y) in enumerate(zip(a.flat, b.flat)) if isinstance(x, torch.Tensor)]
        pairs += [(f"derived {k!r}", bits(a.derived[k]), bits(b.derived[k])) for k in a.derived]
        for nm, x, y in pairs:
            if case.any_nan:
                x, y = canonical_nan16(x), canonical_nan16(y)
            if x.shape != y.shape:
                raise ParityError("return-layout", f"{what}: {nm}: shapes {tuple(x.shape)} vs {tuple(y.shape)}")
            if not torch.equal(x, y):
                d = (x != y).nonzero()
                raise ParityError("values", f"{what}: {nm}: {d.shape[0]} of {x.numel()} cells differ in bits, first at {d[0].tolist()}: kernel "
                                            f"{int(x[tuple(d[0])]):#x}, double {int(y[tuple(d[0])]):#x}")
        return 0.0, 0.0
    ratios = []
    for side, peer, is_double, nm in ((a, real_peer_fn, real_is_double, "kernel"), (b, double_peer_fn, True, "double")):
        try:
            ratios.append(float(case.check(side.call, side.flat, side.derived, peer, is_double)))
        except ParityError:
            raise
        except AssertionError as e:
            raise ParityError("bounded", f"{what}: the {nm} fails the kernel's own check: {e}") from e
    return tuple(ratios)


# ------------------------------------------------------------------------------------------------------------ data and memory
def U(shape, key, scale=1.0):
    """hashed uniform in [-scale, scale) on the CPU (both sides get the same bits by copy)"""
    return syn.hashed_uniform(tuple(shape), "dp." + key, 53) * scale


def ints(shape, key, lim=2):
    """integers in [-lim, lim]"""
    return torch.round(U(shape, key) * (lim + 0.49)).clamp(-lim, lim)


def pow2(shape, key, emin=-2, emax=1):
    """+-2^e, e in [emin, emax]"""
    e = torch.round((U(shape, key + ".e") * 0.5 + 0.5) * (emax - emin) + emin).clamp(emin, emax)
    return torch.where(U(shape, key + ".s") < 0, -1.0, 1.0) * torch.exp2(e)


class Mem:
    """builds the operands and outputs of one call on `device` and keeps the whole buffers for the written-set comparison"""

    def __init__(self, device):
        self.dev = device
        self.watch = {}

    def rows(self, name, t, before=3, after=5, pad=24):
        """a 2-D operand in NaN-poisoned memory (row stride = width + pad)"""
        p = Poisoned(t.to(self.dev), before, after, pad, device=self.dev)
        self.watch[name] = p.buf
        return p.view

    def vec(self, name, v):
        """a contiguous operand followed by NaNs"""
        es = v.element_size()
        buf = torch.full((v.numel() + 24,), NAN_BITS[es], dtype=INT[es], device=self.dev)
        view = buf.view(v.dtype)[:v.numel()]
        view.copy_(v.reshape(-1).to(self.dev))
        self.watch[name] = buf
        return view.view(v.shape)

    def out(self, name, M, n, dtype, c0=0, pad=16, before=2, after=3):
        g = Guarded(M, n, dtype, c0=c0, before=before, after=after, pad=pad, device=self.dev)
        self.watch[name] = g.buf
        return g.view

    def flat(self, name, n, dtype, front=None):
        g = GuardedFlat(n, dtype, front, device=self.dev)
        self.watch[name] = g.buf
        return g.view

    def bytes(self, name, M, D, ldq):
        g = GuardedBytes(M, D, ldq, device=self.dev)
        self.watch[name] = g.buf
        return g.view

    def crop(self, name, t=None, shape=None, dtype=None, margin=(1, 2, 1, 3)):
        """a [C,T,H,W] view inside a larger tensor: poisoned and filled from t, or sentinel-filled (an output)"""
        buf, view, _ = crop(tuple(t.shape) if t is not None else shape, t.dtype if t is not None else dtype, name, margin, poison=t is not None,
                            device=self.dev)
        if t is not None:
            view.copy_(t.to(self.dev))
        self.watch[name] = buf
        return view

    def plain(self, name, t):
        """an operand without guard cells (a weight block the wrapper wants contiguous), still watched"""
        t = t.to(self.dev).contiguous()
        self.watch[name] = t
        return t


def _cpu(t):
    return t.detach().cpu()


# ------------------------------------------------------------------------------------------------------------ cases: copy
CASES = []


def case(op, name, cls, check=None, flippable=False, any_nan=False):
    def deco(build):
        CASES.append(Case(op, name, cls, build, check, flippable, any_nan))
        return build
    return deco


def special_f32(shape, key):
    """arbitrary fp32 data with NaN payloads, infinities, signed zeros, subnormals and values that round up to the next binade"""
    x = U(shape, key, 300.0).reshape(-1)
    sp = torch.tensor([0x7FC00123, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x3F7FFFFF, 0x477FF000, 0x7F7FFFFF],
                      dtype=torch.int64).to(torch.int32).view(F32)
    n = min(sp.numel(), x.numel())
    x[torch.arange(n) * (x.numel() // n)] = sp[:n]
    return x.reshape(shape)


def special_16(shape, key, dtype):
    """arbitrary 16-bit patterns: every exponent, NaN payloads, signed zeros"""
    h = syn.hashed_uniform(tuple(shape), "dp16." + key, 59)
    return torch.round((h * 0.5 + 0.5) * 65535.0).clamp(0, 65535).to(torch.int32).to(torch.int16).view(dtype)


@case("ops.patchify", "c3-special-values", "copy", any_nan=True)
def _(dev):
    m = Mem(dev)
    x = m.plain("x", special_f32((3, 2, 4, 6), "patchify"))
    return Call((x,), {}, m.watch)


@case("ops.patchify", "out-given", "copy", any_nan=True)
def _(dev):
    m = Mem(dev)
    x = m.plain("x", special_f32((16, 1, 2, 2), "patchify.o"))
    o = m.flat("out", 1 * 1 * 1 * 64, BF16).view(1, 64)
    return Call((x,), {"out": o}, m.watch, {0: o})


def _unpatch(dev, with_out, strided):
    m = Mem(dev)
    c, t, h, w = 3, 2, 4, 6
    y = special_16((t * 2 * 3, c * 4), "unpatchify", BF16)
    y = m.rows("y", y, pad=4) if strided else m.plain("y", y)
    if with_out:
        o = m.flat("out", c * t * h * w, BF16).view(c, t, h, w)
        return Call((y, c, t, h, w), {"out": o}, m.watch, {0: o})
    return Call((y, c, t, h, w), {}, m.watch)


case("ops.unpatchify", "no-out", "copy")(lambda dev: _unpatch(dev, False, False))
case("ops.unpatchify", "out-given", "copy")(lambda dev: _unpatch(dev, True, False))
case("ops.unpatchify", "strided-y-out-given", "copy")(lambda dev: _unpatch(dev, True, True))


def _copy3d(dev):
    m = Mem(dev)
    src = m.rows("src", special_16((2 * 5, 40), "copy3d", BF16), pad=8)          # 2 batches of 5 rows, ld 48
    dst = m.out("dst", 2 * 7, 24, BF16, c0=8, pad=8)                             # ld 40: 3 of 7 rows per batch, 24 columns written
    return Call((src, dst, 2, 3, 24, 5 * 48, 48, 7 * 40, 40), {}, m.watch, {0: dst})


case("ops.copy3d", "batched-strided", "copy")(_copy3d)
case("sp.copy3d", "batched-strided", "copy")(_copy3d)


@case("vae_ops.copy4d_", "crop-to-crop", "copy")
def _(dev):
    m = Mem(dev)
    src = m.crop("src", special_16((3, 2, 3, 5), "copy4d", F16))
    dst = m.crop("dst", shape=(3, 2, 3, 5), dtype=F16, margin=(2, 1, 3, 1))
    return Call((src, dst), {}, m.watch, {0: dst})


@case("ops.broadcast_row_", "padded-dst", "copy")
def _(dev):
    m = Mem(dev)
    src = m.vec("src", special_16((40,), "bcast", BF16))
    dst = m.out("dst", 5, 40, BF16, c0=8)
    return Call((src, dst), {}, m.watch, {0: dst})


@case("vae_ops.latent_tile", "strided-view-cpad", "copy")
def _(dev):
    m = Mem(dev)
    z = m.crop("z", special_f32((5, 2, 3, 4), "latent"))
    return Call((z, 8), {}, m.watch)


@case("vae_ops.transpose_16b", "ragged-tile", "copy")
def _(dev):
    m = Mem(dev)
    src = m.rows("src", special_16((37, 24), "transpose", F16), pad=8)
    dst = m.out("dst", 24, 37, F16, c0=8, pad=11)
    return Call((src, dst), {}, m.watch, {0: dst})


@case("vae_ops.temporal_nearest_up", "s2", "copy")
def _(dev):
    m = Mem(dev)
    x = m.rows("x", special_16((3 * 5, 16), "tnear", F16), pad=8)
    return Call((x, 3, 5, 2), {}, m.watch)


def finite_f16(shape, key, scale=4.0):
    return U(shape, key, scale).to(F16)


@case("vae_ops.temporal_linear_up", "s2-and-ends", "copy")
def _(dev):
    m = Mem(dev)
    x = finite_f16((4 * 5, 16), "tlin")
    x[0, :4] = torch.tensor([-0.0, 0.0, 65504.0, 2.0 ** -24])
    x = m.rows("x", x, pad=8)
    return Call((x, 4, 5, 2), {}, m.watch)


@case("vae_ops.temporal_linear_up", "s4-one-frame", "copy")
def _(dev):
    m = Mem(dev)
    x = m.rows("x", finite_f16((1 * 3, 8), "tlin1"), pad=8)
    return Call((x, 1, 3, 4), {}, m.watch)


@case("ops.fp8_dequant", "all-256-codes", "copy", any_nan=True)
def _(dev):
    m = Mem(dev)
    w8 = m.plain("w8", torch.arange(256, dtype=torch.int64).to(torch.uint8).view(FP8).reshape(4, 64))
    sc = m.vec("scale", torch.tensor([0.0123], dtype=BF16))
    o = m.flat("out", 256, BF16).view(4, 64)
    return Call((w8, sc, o), {}, m.watch, {0: o})


def _quant_rows():
    x = RB.data_rows("massive", 5, 520, "dp.quant")
    x[3] = 0
    x[4, :] = 0
    x[4, 7] = 2.0 ** -125
    return x


@case("ops.quant_rows_fp8", "given-outputs-long-scale", "copy")
def _(dev):
    m = Mem(dev)
    x = m.rows("x", _quant_rows(), pad=8)
    q = m.bytes("out_q", 5, 520, 544)
    s = m.flat("out_scale", 5 + 3, F32)                      # out_scale longer than m: rows behind m keep their bits
    return Call((x,), {"out_q": q, "out_scale": s}, m.watch, {0: q, 1: s})


@case("ops.quant_rows_fp8", "allocating", "copy")
def _(dev):
    m = Mem(dev)
    x = m.rows("x", RB.data_rows("control", 4, 512, "dp.quant2"), pad=8)
    return Call((x,), {}, m.watch)


# ------------------------------------------------------------------------------------------------------------ cases: exact
GEMM_EXACT = [("B1", 5, 64, 64), ("B2", 5, 264, 128), ("B3", 5, 264, 192)]     # the cheapest shape of each gemm_path (N <= 128; N > 128 and K < 192; K >= 192)


def _gemm_exact_operands(N, K, M, key, flip, dt=BF16):
    a, w, b = ints((M, K), key + ".a").to(dt), ints((N, K), key + ".w").to(dt), ints((N,), key + ".b", 9).to(dt)
    if flip:
        a, w = a.flip(-1), w.flip(-1)
    return a, w, b


def _gemm_exact(dev, flip, path, M, N, K, form):
    m = Mem(dev)
    a, w, b = _gemm_exact_operands(N, K, M, f"gemm.{path}", flip)
    A, W, B = m.rows("a", a), m.rows("w", w, 2, 7, 40), m.vec("bias", b)
    if form == "bias":
        o = m.out("out", M, N, BF16, c0=8)
        return Call((A, W, B), {"out": o}, m.watch, {0: o})
    if form == "alloc":
        return Call((A, W, B), {"act": 0}, m.watch)
    if form == "wide-out":                       # out wider than n0: its columns behind N keep their bits
        o = m.out("out", M, N + 16, BF16, c0=8)
        return Call((A, W), {"out": o}, m.watch, {0: o})
    if form == "split":                          # out1 behind an offset, out narrower than N
        ns = 8 if N <= 64 else 136
        o, o1 = m.out("out", M, ns, BF16, c0=0), m.out("out1", M, N - ns, BF16, c0=24)
        return Call((A, W, B), {"out": o, "n_split": ns, "out1": o1}, m.watch, {0: o})
    gate = m.vec("gate", (2.0 * ints((N,), f"gemm.{path}.g", 3) + 1.0).to(BF16))            # odd integers: y * gate needs its own rounding
    res = ints((M, N), f"gemm.{path}.r", 200).to(BF16)
    if form == "gate-in-place":                  # res is out
        r = m.rows("res", res, 1, 4, 16)
        return Call((A, W, B), {"out": r, "gate": gate, "res": r}, m.watch, {0: r})
    if form == "gate":
        r, o = m.rows("res", res, 1, 4, 16), m.out("out", M, N, BF16, c0=8)
        return Call((A, W, B), {"out": o, "gate": gate, "res": r}, m.watch, {0: o})
    if form == "res-no-gate":                    # out = bf16(res + y): one rounding
        r, o = m.rows("res", res, 1, 4, 16), m.out("out", M, N, BF16, c0=8)
        return Call((A, W, B), {"out": o, "res": r}, m.watch, {0: o})
    if form == "split+gate+res":                 # res and gate span all N columns: those of out1 take them too
        r, o, o1 = m.rows("res", res, 1, 4, 16), m.out("out", M, 136, BF16), m.out("out1", M, N - 136, BF16, c0=24)
        return Call((A, W, B), {"out": o, "n_split": 136, "out1": o1, "gate": gate, "res": r}, m.watch, {0: o})
    raise KeyError(form)


for _p, _M, _N, _K in GEMM_EXACT:
    for _form in ("bias", "split", "gate-in-place") + (("alloc", "wide-out", "gate", "res-no-gate", "split+gate+res") if _p == "B3" else ()):
        case("ops.gemm", f"{_p}-{_form}", "exact", flippable=True)(
            lambda dev, flip=False, a=(_p, _M, _N, _K, _form): _gemm_exact(dev, flip, *a))


@case("ops.gemm", "leading-dims", "exact", flippable=True)
def _(dev, flip=False):
    m = Mem(dev)
    a, w, b = _gemm_exact_operands(64, 64, 6, "gemm.lead", flip)
    A = m.rows("a", a).unflatten(0, (2, 3))                  # [2, 3, K] with uniformly strided rows
    return Call((A, m.rows("w", w), m.vec("bias", b)), {}, m.watch)


def _gemm_fp8_exact(dev, flip, form):
    m = Mem(dev)
    M, N, K = 5, 72, 384
    a, w, b = _gemm_exact_operands(N, K, M, "gemm8", flip, F32)
    A, W = m.rows("a_q", a.to(FP8), pad=32), m.rows("w_q", w.to(FP8), 2, 7, 48)
    asc = m.vec("a_scale", pow2((M + 3,), "gemm8.as", -3, 2).abs())[:M + 3]
    ws = m.vec("w_scale", torch.tensor([0.5], dtype=BF16))
    B = m.vec("bias", b.to(BF16))
    if form == "bias":
        o = m.out("out", M, N, BF16, c0=8)
        return Call((A, asc, W, ws, B), {"out": o}, m.watch, {0: o})
    if form == "alloc":
        return Call((A, asc, W, ws), {}, m.watch)
    if form == "split":
        o, o1 = m.out("out", M, 16, BF16), m.out("out1", M, N - 16, BF16, c0=24)
        return Call((A, asc, W, ws, B), {"out": o, "n_split": 16, "out1": o1, "act1": 0}, m.watch, {0: o})
    gate = m.vec("gate", (2.0 * ints((N,), "gemm8.g", 3) + 1.0).to(BF16))
    r = m.rows("res", ints((M, N), "gemm8.r", 200).to(BF16), 1, 4, 16)
    if form == "res-no-gate":
        o = m.out("out", M, N, BF16, c0=8)
        return Call((A, asc, W, ws, B), {"out": o, "res": r}, m.watch, {0: o})
    if form == "split+gate+res":
        o, o1 = m.out("out", M, 16, BF16), m.out("out1", M, N - 16, BF16, c0=24)
        return Call((A, asc, W, ws, B), {"out": o, "n_split": 16, "out1": o1, "gate": gate, "res": r}, m.watch, {0: o})
    return Call((A, asc, W, ws, B), {"out": r, "gate": gate, "res": r}, m.watch, {0: r})


for _form in ("bias", "alloc", "split", "gate-in-place", "res-no-gate", "split+gate+res"):
    case("ops.gemm_fp8", f"Q-{_form}", "exact", flippable=True)(lambda dev, flip=False, f=_form: _gemm_fp8_exact(dev, flip, f))


def _smallm_exact(dev, flip, M, form):
    m = Mem(dev)
    N, K = 5, 520
    a, w, b = _gemm_exact_operands(N, K, M, f"smallm.{M}", flip)
    X, W = m.rows("x", a, pad=8), m.plain("w", w)
    if form == "addend":
        o = m.out("out", M, N, BF16, pad=3)
        add = m.out("addend", M, N, BF16, pad=3)             # the geometry of the output buffer
        add.copy_(ints((M, N), "smallm.add", 50).to(BF16))
        return Call((X, W, m.vec("bias", b)), {"out": o, "addend": add}, m.watch, {0: o})
    return Call((X, W), {}, m.watch)


for _M in (1, 4):
    for _form in ("plain", "addend"):
        case("ops.linear_smallm", f"M{_M}-{_form}", "exact", flippable=True)(lambda dev, flip=False, a=(_M, _form): _smallm_exact(dev, flip, *a))


def _gemm_f16_exact(dev, flip, form):
    m = Mem(dev)
    M, N, K = 5, 72, 192
    a, w, b = _gemm_exact_operands(N + 8, K + 64, M, "gemmf16", False, F16)
    if flip:                                     # only the K columns the call multiplies
        a[:, :K], w[:, :K] = a[:, :K].flip(-1), w[:, :K].flip(-1)
    A, W, B = m.rows("a", a), m.rows("w", w, 2, 7, 40), m.vec("bias", b)
    if form == "out_f32":
        o = m.out("out", M, N, F32, c0=8)
        return Call((A, W, B), {"out": o, "out_f32": True, "n": N, "k": K}, m.watch, {0: o})
    if form == "res":
        r, o = m.rows("res", ints((M, N), "gemmf16.r", 200).to(F16), 1, 4, 16), m.out("out", M, N, F16, c0=8)
        return Call((A, W, B), {"out": o, "res": r, "n": N, "k": K}, m.watch, {0: o})
    return Call((A, W), {}, m.watch)              # whole operands, allocating


for _form in ("out_f32", "res", "alloc"):
    case("vae_ops.gemm_f16", _form, "exact", flippable=True)(lambda dev, flip=False, f=_form: _gemm_f16_exact(dev, flip, f))


def _conv_operands(rows, cin, cout, key, flip, ld_pad=8):
    x, w, b = ints((rows, cin), key + ".x").to(F16), ints((cout, 27, cin), key + ".w", 1).to(F16), ints((cout,), key + ".b", 9).to(F16)
    if flip:
        x, w = x.flip(-1), w.flip(-1)
    return x, w, b


def gn_weights(C, key):
    return (1 + 0.1 * U((C,), key + ".gw")).to(F16), (0.5 * U((C,), key + ".gb")).to(F16)


def _post_gn(ret, call, peer):
    """what groupnorm_affine_from_stats makes of the statistics, judged by the GroupNorm check on the side's own stored output.
    The two affines are not compared bit for bit, exact data or not: an entry's C2 = sum (x - S / k)^2 is not an integer, it is
    rounded to fp32 per partial row, and the kernel keeps one row per 64-row block (from pivot-shifted sums) where the double keeps
    a single row over all M - the fp64 fold sees different fp32 inputs and sc / sh may differ in their last bit.  The stored output,
    from which both sides take their statistics, IS compared bit for bit."""
    out, st = ret
    w, b = (t.to(out.device) for t in gn_weights(out.shape[1], "conv"))
    aff = peer("vae_ops.groupnorm_affine_from_stats")(st, w, b)
    from tests.test_gpu_groupnorm_conditioning import AFFINE_TOL, affine_error
    err, _ = affine_error(_cpu(out), _cpu(aff), w.cpu(), b.cpu())
    assert float(err) <= AFFINE_TOL, f"affine from the epilogue statistics: error {float(err):.3e} above {AFFINE_TOL}"
    return {}


def _conv_exact(dev, flip, T, H, W, cin, cout, up_t, up_hw, form):
    m = Mem(dev)
    src = ((T + 1) // 2 if up_t else T, H >> int(up_hw), W >> int(up_hw))
    x, w, b = _conv_operands(src[0] * src[1] * src[2], cin, cout, f"conv.{cin}.{cout}", flip)
    X, Wt, B = m.rows("x", x, pad=8), m.plain("w_taps", w), m.vec("bias", b)
    kw = {"up_t": up_t, "up_hw": up_hw}
    if form == "res":
        r = m.rows("res", ints((T * H * W, cout), "conv.res", 200).to(F16), 1, 4, 16)
        o = m.out("out", T * H * W, cout, F16, c0=8)
        return Call((X, Wt, B, T, H, W, cin, cout), dict(kw, res=r, out=o), m.watch, {0: o})
    if form == "gn_stats":
        return Call((X, Wt, B, T, H, W, cin, cout), dict(kw, gn_stats=True), m.watch, post=_post_gn)
    return Call((X, Wt, B, T, H, W, cin, cout), kw, m.watch)


for _nm, _a in {"plain": (3, 5, 7, 64, 64, False, False, "plain"), "up_t": (5, 4, 6, 128, 64, True, False, "plain"),
                "up_hw": (2, 6, 10, 64, 128, False, True, "plain"), "up_t+up_hw": (3, 4, 8, 128, 128, True, True, "plain"),
                "res": (2, 4, 8, 128, 64, False, False, "res"), "gn_stats": (3, 5, 7, 64, 64, False, False, "gn_stats")}.items():
    case("vae_ops.conv3d_causal", _nm, "exact", flippable=True)(lambda dev, flip=False, a=_a: _conv_exact(dev, flip, *a))


def _subpixel_exact(dev, flip, up_t):
    from hunyuanvideo_efficiency_amd import vae_ops
    m = Mem(dev)
    sT, sH, sW, cin, cout = 2, 2, 3, 256, 136
    x = ints((sT * sH * sW, cin), "subpix.x").to(F16)
    w = ints((cout, cin, 3, 3, 3), "subpix.w", 1).to(F16)
    b = ints((cout,), "subpix.b", 9).to(F16)
    if flip:
        x, w = x.flip(-1), w.flip(1)
    w_sub, table, ntap = vae_ops.subpixel_weights(w, up_t)           # sums of at most 8 weights of size 1: exact in fp16
    return Call((m.rows("x", x, pad=8), m.plain("w_sub", w_sub), m.plain("table", table), ntap, m.vec("bias", b), sT, sH, sW, cin, cout, up_t),
                {}, m.watch)


for _up in (False, True):
    case("vae_ops.conv3d_upsampled_subpixel", f"up_t={_up}", "exact", flippable=True)(lambda dev, flip=False, u=_up: _subpixel_exact(dev, flip, u))


def _strided_exact(dev, flip, stride):
    m = Mem(dev)
    sT, sH, sW, cin, cout = 3, 5, 6, 64, 64
    x, w, b = _conv_operands(sT * sH * sW, cin, cout, "strided", flip)
    T, H, W = CB.out_grid((sT, sH, sW), stride)
    o = m.out("out", T * H * W, cout, F16, c0=8)
    return Call((m.rows("x", x, pad=8), m.plain("w_taps", w), m.vec("bias", b), sT, sH, sW, cin, cout), {"stride": stride, "out": o}, m.watch, {0: o})


for _s in ((2, 2, 2), (1, 2, 2), (2, 1, 1), (1, 1, 1)):
    case("vae_ops.conv3d_causal_strided", "stride-" + "".join(map(str, _s)), "exact", flippable=True)(
        lambda dev, flip=False, s=_s: _strided_exact(dev, flip, s))


def _cout4_exact(dev, flip, ldo):
    from hunyuanvideo_efficiency_amd import vae_ops
    m = Mem(dev)
    T, H, W, cin, cout = 3, 5, 7, 64, 3
    x = ints((T * H * W, cin), "cout4.x").to(F16)
    w = ints((cout, cin, 3, 3, 3), "cout4.w", 1).to(F16)
    b = ints((cout,), "cout4.b", 9).to(F16)
    if flip:
        x, w = x.flip(-1), w.flip(1)
    o = m.out("out", T * H * W, min(ldo, 8), F16, pad=ldo - min(ldo, 8), before=8, after=3)      # 8 rows in front: the view stays 16-byte aligned
    assert o.stride(0) == ldo and o.data_ptr() % 16 == 0
    return Call((m.rows("x", x, pad=8), None, False, m.plain("w_frag", vae_ops.cout4_weight_fragments(w)), m.vec("bias", b), T, H, W, cin, cout),
                {"out": o}, m.watch, {0: o})


for _ldo in (8, 16, 3):
    case("vae_ops.conv_cout4", f"no-affine-ldo{_ldo}", "exact", flippable=True)(lambda dev, flip=False, l=_ldo: _cout4_exact(dev, flip, l))


@case("vae_ops.groupnorm_apply", "no-silu-pow2-scale", "exact")
def _(dev):
    m = Mem(dev)
    x = m.rows("x", ints((37, 64), "gnapply.x", 100).to(F16), pad=8)
    aff = m.plain("affine", torch.stack([pow2((64,), "gnapply.sc", -3, 2), ints((64,), "gnapply.sh", 20)], 1).float())
    o = m.out("out", 37, 64, F16, c0=8)
    return Call((x, aff, False), {"out": o}, m.watch, {0: o})


@case("vae_ops.temporal_avg_pool", "k2-s2", "exact")
def _(dev):
    m = Mem(dev)
    return Call((m.rows("x", ints((5 * 3, 16), "tavg2", 500).to(F16), pad=8), 5, 3, 2, 2), {}, m.watch)


@case("vae_ops.temporal_avg_pool", "k3-s2", "exact")
def _(dev):
    # an integer sum S times fp32(1/3) is within 2^-24 relative of S / 3, which is never near an fp16 rounding tie (n + 1/3 and n + 2/3
    # lie 1/3 of an fp16 spacing from the nearest value at every spacing >= 2^-10 used here): every order of the exact sum gives these bits
    m = Mem(dev)
    return Call((m.rows("x", ints((5 * 3, 16), "tavg3", 300).to(F16), pad=8), 5, 3, 3, 2), {}, m.watch)


@case("ops.euler_step_", "pow2-dt", "exact")
def _(dev):
    m = Mem(dev)
    s = m.flat("sample", 1027, F32)
    s.copy_((ints((1027,), "euler.s", 4000) * 0.125).to(dev))
    v = m.vec("model_out", ints((1027,), "euler.v", 200).to(BF16))
    return Call((s, v, -0.25), {}, m.watch, {0: s})


def _masked_mean_exact(dev, masked):
    m = Mem(dev)
    L = 16 if masked else 8
    x = m.plain("x", ints((L, 40), "mmean.x", 100).to(BF16))
    mask = None
    if masked:
        mk = torch.zeros(L, dtype=I32)
        mk[[0, 1, 2, 5, 7, 8, 11, 15]] = 1
        mask = m.plain("mask", mk)
    return Call((x, mask), {}, m.watch)


case("ops.masked_mean", "no-mask-8-rows", "exact")(lambda dev: _masked_mean_exact(dev, False))
case("ops.masked_mean", "mask-8-of-16", "exact")(lambda dev: _masked_mean_exact(dev, True))


def _softmax_exact(dev, causal):
    m = Mem(dev)
    rows, cols, cols_pad = 8, 8, 16
    s = m.rows("S", torch.full((rows, cols_pad), 4.0), pad=8)
    o = m.out("out", rows, cols_pad, F16, c0=8)
    return Call((s, cols, cols_pad, 0.5), {"out": o, "causal_block": 4 if causal else 0}, m.watch, {0: o})


case("vae_ops.softmax_rows", "constant-8-cols", "exact")(lambda dev: _softmax_exact(dev, False))
case("vae_ops.softmax_rows", "constant-causal-4-8", "exact")(lambda dev: _softmax_exact(dev, True))


def census(n_q, n_kv, H, key):
    """q = +0, k >= 0 (every score is +0, every p exactly 1), integer V: out = column sums / n_kv"""
    q = torch.zeros(n_q, H * 128, dtype=BF16)
    k = ints((n_kv, H * 128), key + ".k", 2).abs().to(BF16)
    v = ints((n_kv, H * 128), key + ".v", 3).to(BF16)
    return q, k, v


def _fused(m, q, k, v, H):
    """column slices of one fused [rows, 3 H 128 + 64] buffer, as the blocks pass them (q shorter than k / v: rows behind n_q are pad)"""
    d, rows = H * 128, max(q.shape[0], k.shape[0])
    t = torch.full((rows, 3 * d + 40), float("nan"), dtype=BF16)
    t[:q.shape[0], :d], t[:k.shape[0], d:2 * d], t[:k.shape[0], 2 * d:3 * d] = q, k, v
    buf = m.rows("qkv", t, pad=24)
    return buf[:q.shape[0], :d], buf[:k.shape[0], d:2 * d], buf[:k.shape[0], 2 * d:3 * d]


def _attn_fwd_census(dev, n_q, n_kv, **kw):
    m = Mem(dev)
    H = 2
    q, k, v = _fused(m, *census(n_q, n_kv, H, f"census.{n_kv}"), H)
    o = m.out("out", n_q + 2, H * 128, BF16, pad=64)[:n_q]          # rows behind n_q and the pad columns keep their bits
    return Call((q, k, v, o, H), kw, m.watch, {0: o})


case("ops.attn_fwd", "census-321x64-no-split-workspace", "exact")(lambda dev: _attn_fwd_census(dev, 321, 64, kv_split_workspace=False))
for _nq, _nkv in ((1, 1), (321, 64), (1, 256)):
    case("ops.attn_fwd", f"census-{_nq}x{_nkv}", "exact")(lambda dev, a=(_nq, _nkv): _attn_fwd_census(dev, *a))
    case("sp.attn_fwd", f"census-{_nq}x{_nkv}", "exact")(lambda dev, a=(_nq, _nkv): _attn_fwd_census(dev, *a))


def _parts_attrs(parts):
    return {"o": parts.o[:parts.used], "ml": parts.ml[:parts.used],
            "shape": torch.tensor(list(parts.o.shape) + list(parts.ml.shape) + [parts.n_slots, parts.n_q, parts.n_heads, parts.used]),
            "dtype": torch.tensor([parts.o.dtype == F32, parts.ml.dtype == F32])}


def _attn_partial_census(dev, n_q, n_kv, splits):
    m = Mem(dev)
    H = 2
    q, k, v = _fused(m, *census(n_q, n_kv, H, f"census.{n_kv}"), H)
    mk = real_fn if str(dev) != "cpu" else double_fn
    parts = mk("sp.attn_partials")(splits + 1, n_q, H, dev)
    parts.o.fill_(7.0), parts.ml.fill_(7.0)                          # the unused slot keeps this
    m.watch["part_o"], m.watch["part_ml"] = parts.o, parts.ml
    args = (q, k, v, parts, H, splits)
    return Call(args, {}, m.watch, post=lambda ret, call, peer: _parts_attrs(call.args[3]))


for _nq, _nkv, _sp in ((1, 1, 1), (321, 65, 1), (1, 449, 1), (321, 129, 2), (1, 191, 2)):
    for _space in ("ops", "sp"):
        case(f"{_space}.attn_partial", f"census-{_nq}x{_nkv}-splits{_sp}", "exact")(
            lambda dev, a=(_nq, _nkv, _sp): _attn_partial_census(dev, *a))


def _attn_merge_exact(dev):
    m = Mem(dev)
    n_q, H = 5, 2
    mk = real_fn if str(dev) != "cpu" else double_fn
    parts = mk("sp.attn_partials")(3, n_q, H, dev)
    parts.o.copy_(ints((3, n_q, H, 128), "merge.o", 200).to(dev))
    parts.ml[..., 0], parts.ml[..., 1] = 0.0, 64.0                   # m = 0, l = 64 in each of the two used slots: a row sum of 128
    parts.used = 2
    m.watch["part_o"], m.watch["part_ml"] = parts.o, parts.ml
    o = m.out("out", n_q, H * 128, BF16, pad=64)
    return Call((parts, o), {}, m.watch, {0: o})


case("ops.attn_merge", "two-slots-of-64", "exact")(_attn_merge_exact)
case("sp.attn_merge", "two-slots-of-64", "exact")(_attn_merge_exact)


@case("sp.attn_partials", "attributes", "exact")
def _(dev):
    return Call((2, 3, 4, dev), {}, {}, post=lambda ret, call, peer: {
        "shape": torch.tensor(list(ret.o.shape) + list(ret.ml.shape) + [ret.n_slots, ret.n_q, ret.n_heads, ret.used]),
        "dtype": torch.tensor([ret.o.dtype == F32, ret.ml.dtype == F32])})


# ------------------------------------------------------------------------------------------------------------ cases: bounded
def _out0(flat):
    return _cpu(flat[0])


LN_MODES = ["shift+scale", "scale", "shift", "neither", "affine"]


def _ln_operands(D, mode, key):
    shift = RB._u((D,), key + ".shift", 0.5).to(BF16) if mode in ("shift+scale", "shift", "affine") else None
    if mode == "affine":
        mul = (1.0 + RB._u((D,), key + ".w", 0.3)).to(BF16)
    else:
        mul = RB._u((D,), key + ".scale", 0.5).to(BF16) if mode in ("shift+scale", "scale") else None
    return shift, mul


def _ln(dev, D, mode, cls, fp8):
    m = Mem(dev)
    M = 5
    x = RB.data_rows(cls, M, D, f"dp.ln.{D}")
    shift, mul = _ln_operands(D, mode, f"dp.ln.{D}.{mode}")
    X = m.rows("x", x)
    sv, mv = (None if t is None else m.vec(n, t) for n, t in (("shift", shift), ("scale", mul)))
    ref = (x, shift, mul, mode == "affine", (X, sv, mv))
    if fp8:
        q, s = m.bytes("out_q", M, D, (D + 15) // 16 * 16 + 16), m.flat("out_scale", M, F32)
        return Call((X, sv, mv), {"out_q": q, "out_scale": s}, m.watch, {0: q, 1: s}, ref)
    o = m.out("out", M, D, BF16)
    return Call((X, sv, mv), {"out": o, "affine": mode == "affine"}, m.watch, {0: o}, ref)


def _ln_check(call, flat, derived, peer, is_double):
    x, shift, mul, affine, _ = call.ref
    y64, bound = RB.ln_ref(x, shift, mul, affine=affine)
    return RB.check(_out0(flat), y64, bound, "ln_modulate")


def _ln_fp8_check(call, flat, derived, peer, is_double):
    """the side's own bf16 LayerNorm output inside the LayerNorm bound, and the codes / scales the oracle's quantisation of THAT output"""
    x, shift, mul, _, (X, sv, mv) = call.ref
    y = _cpu(peer("ops.ln_modulate")(X, sv, mv))
    y64, bound = RB.ln_ref(x, shift, mul)
    r = RB.check(y, y64, bound, "ln_modulate_fp8: the bf16 rows")
    q_ref, s_ref = R.fp8_quant_rows(y)
    assert torch.equal(bits(flat[1]), bits(s_ref.reshape(-1))), "ln_modulate_fp8: row scales differ from amax(bf16 output) * (1/448)"
    assert torch.equal(bits(flat[0]), bits(q_ref.to(FP8))), "ln_modulate_fp8: codes differ from the oracle's quantisation of the bf16 output"
    return r


for _D in (512, 520):                            # one D on each side of a MAXC boundary
    for _mode in LN_MODES:
        case("ops.ln_modulate", f"D{_D}-{_mode}", "bounded", _ln_check)(
            lambda dev, a=(_D, _mode, "massive" if _mode == "affine" else "control", False): _ln(dev, *a))
    case("ops.ln_modulate_fp8", f"D{_D}-shift+scale", "bounded", _ln_fp8_check)(lambda dev, D=_D: _ln(dev, D, "shift+scale", "control", True))


def _qk(dev, H, scatter):
    m = Mem(dev)
    n_rows, n_rope = 5, 4
    key = f"dp.qk.{H}"
    row, x, w, qw, kw = RB.qk_case("control", H, n_rows, key)
    cos, sin = RB.rope_tables_independent(n_rows, key)
    k_off = H * 128 + 128
    t = row[:, :3 * H * 128 + 40].clone()
    t[:, H * 128:k_off] = float("nan")
    Q = m.rows("qkv", t)
    cp, sp = cos.clone(), sin.clone()
    cp[n_rope:], sp[n_rope:] = float("nan"), float("nan")
    args = (Q, m.vec("q_weight", qw), m.vec("k_weight", kw), m.plain("cos", cp), m.plain("sin", sp), n_rope, H, k_off)
    ref = (x, w, cos, sin, n_rope, H, k_off)
    if not scatter:
        return Call(args, {}, m.watch, {0: Q}, ref)
    hpb = 2 if H > 1 else 1
    nblk = 2 * H // hpb
    buf = torch.full((nblk, n_rows + 3, hpb * 128 + 64), SENT[2], dtype=torch.int16, device=dev)
    m.watch["out"] = buf
    dst = buf.view(BF16)[:, 1:1 + n_rows, :hpb * 128].permute(1, 0, 2)           # 3-D scatter view [rows, blocks, hpb * 128]
    return Call(args, {"out": dst}, m.watch, {0: dst}, ref)


def _qk_check(call, flat, derived, peer, is_double):
    x, w, cos, sin, n_rope, H, k_off = call.ref
    o = _out0(flat)
    got = (o.reshape(o.shape[0], 2 * H, 128) if o.dim() == 3 else
           torch.cat([o[:, :H * 128], o[:, k_off:k_off + H * 128]], 1).reshape(o.shape[0], 2 * H, 128))
    y64, bound, amb, amb_bound = RB.qknorm_ref(x, w, cos, sin, n_rope)
    assert bool(torch.isfinite(got.float()).all()), "qknorm_rope: not finite"
    r = RB.check(got.reshape(-1, 128), y64.reshape(-1, 128), bound.reshape(-1, 128), "qknorm_rope", skip=amb.reshape(-1, 128))
    assert bool(((got.double() - y64).abs() <= amb_bound)[amb].all()), "qknorm_rope: an ambiguous element is more than 2 ulp off"
    return r


for _H in (1, 9):
    case("ops.qknorm_rope_", f"H{_H}-in-place", "bounded", _qk_check)(lambda dev, H=_H: _qk(dev, H, False))
    case("ops.qknorm_rope_", f"H{_H}-scatter", "bounded", _qk_check)(lambda dev, H=_H: _qk(dev, H, True))


@case("ops.timestep_embedding", "dim256", "bounded",
      lambda call, flat, d, peer, is_double: RB.check(_out0(flat), *RB.timestep_ref(call.ref, 256), "timestep_embedding"))
def _(dev):
    m = Mem(dev)
    t = torch.tensor(RB.TS, dtype=F32)
    return Call((m.vec("t", t), 256), {}, m.watch, ref=t)


def _gemm_act(dev, kind, act):
    m = Mem(dev)
    M, N = 5, 264
    K = 384 if kind == "fp8" else 192
    key = f"dp.act.{kind}"
    a, w, b = RB._u((M, K), key + ".a", 0.5), RB._u((N, K), key + ".w", 1.0 / math.sqrt(K)), RB._u((N,), key + ".b", 0.05).to(BF16)
    o = m.out("out", M, N, BF16, c0=8)
    if kind == "fp8":
        ws = (w.abs().max() / 448.0).to(BF16)
        w8 = (w / ws.float()).clamp(-448, 448).to(FP8)
        asc = a.abs().amax(1).clamp(min=1e-12) / 448.0
        a8 = (a / asc[:, None]).clamp(-448, 448).to(FP8)
        ref = EB.gemm_ref(a8.double() * asc.double()[:, None], w8.double() * ws.double(), b)
        args = (m.rows("a_q", a8, pad=32), m.vec("a_scale", asc), m.rows("w_q", w8, 2, 7, 48), m.vec("w_scale", ws.reshape(1)), m.vec("bias", b))
    else:
        a, w = a.to(BF16), w.to(BF16)
        ref = EB.gemm_ref(a, w, b)
        args = (m.rows("a", a), m.rows("w", w, 2, 7, 40), m.vec("bias", b))
    return Call(args, {"out": o, "act": act}, m.watch, {0: o}, (ref, args, kind, act))


def act_ratio(fn, got, y, what):
    """the activation site's check of tests/test_gpu_activation_domain.py: got against the fp64 reference and bound of
    activation_bounds.act_ref (ulp + E32 + FLOOR) on the 16-bit pre-activation y the same side produced"""
    y64, _, bound = ACT.act_ref(fn, y, y.dtype)
    return ACT.check(got, y64, bound, what)


def _gemm_act_check(call, flat, derived, peer, is_double):
    """the side's plain product y inside the fp64 GEMM bound, and its activation inside activation_bounds' bound on that y"""
    ref, args, kind, act = call.ref
    y = _cpu(peer("ops.gemm_fp8" if kind == "fp8" else "ops.gemm")(*args))
    r = EB.check(y, ref, BF16, f"gemm {kind}: the plain product", worst_case=kind == "fp8")
    fn = "gelu" if act == 1 else "silu"
    return max(r, act_ratio(fn, _out0(flat), y, f"gemm {kind}: the {fn} epilogue on the side's own product"))


for _kind in ("bf16", "fp8"):
    for _act, _nm in ((1, "gelu"), (2, "silu")):
        case("ops.gemm_fp8" if _kind == "fp8" else "ops.gemm", f"{_nm}-epilogue", "bounded", _gemm_act_check)(
            lambda dev, a=(_kind, _act): _gemm_act(dev, *a))


def _smallm_silu(dev, silu_in, silu_out):
    m = Mem(dev)
    M, N, K = 3, 5, 520
    x, w, b = RB.gemv_operands(M, N, K, "dp.gemv")
    x = RB.tie_free_for_silu(x)
    X, W, B = m.rows("x", x, pad=8), m.plain("w", w), m.vec("bias", b)
    return Call((X, W, B), {"silu_in": silu_in, "silu_out": silu_out}, m.watch, ref=(x, w, b, X, W, B, silu_in, silu_out))


def _smallm_check(call, flat, derived, peer, is_double):
    x, w, b, X, W, B, silu_in, silu_out = call.ref
    silu = lambda v: RB.silu64(v).to(BF16)
    ref = EB.gemm_ref(silu(x) if silu_in else x, w, b)
    y = _cpu(peer("ops.linear_smallm")(X, W, B, silu_in=silu_in))
    r = EB.check(y, ref, BF16, "linear_smallm: the product")
    if silu_out:
        r = max(r, act_ratio("silu", _out0(flat), y, "linear_smallm: silu_out on the side's own product"))
    return r


for _si, _so in ((True, False), (False, True), (True, True)):
    case("ops.linear_smallm", f"silu_in={_si}-silu_out={_so}", "bounded", _smallm_check)(lambda dev, a=(_si, _so): _smallm_silu(dev, *a))


def _mmean_random(dev):
    m = Mem(dev)
    x = RB._u((11, 40), "dp.mmean").to(BF16)
    mk = torch.tensor([1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], dtype=I32)
    return Call((m.plain("x", x), m.plain("mask", mk)), {}, m.watch, ref=(x, mk))


case("ops.masked_mean", "random-7-of-11", "bounded",
     lambda call, flat, d, peer, is_double: EB.check(_out0(flat)[None], RB.masked_mean_ref(*call.ref), BF16, "masked_mean"))(_mmean_random)


def gn_x(M, C, kind, key):
    u = U((M, C), key)
    if kind == "control":
        return (0.3 + u * (2.0 * math.sqrt(3.0))).to(F16)
    g = torch.arange(C) // (C // 32)
    return (torch.where((g % 4) < 2, 1.0, -1.0) * 10.0 + u * math.sqrt(3.0)).to(F16)          # every group at +-10 with unit variance


def _gn_affine(dev, kind):
    m = Mem(dev)
    x = gn_x(105, 64, kind, "dp.gn." + kind)
    w, b = gn_weights(64, "gn")
    return Call((m.rows("x", x, pad=8), m.vec("weight", w), m.vec("bias", b)), {}, m.watch, ref=(x, w, b))


def _gn_affine_check(call, flat, derived, peer, is_double):
    from tests.test_gpu_groupnorm_conditioning import AFFINE_TOL, affine_error
    x, w, b = call.ref
    aff = _out0(flat)
    assert bool(torch.isfinite(aff).all()), "groupnorm_affine: non-finite affine"
    err, _ = affine_error(x, aff, w, b)
    assert float(err) <= AFFINE_TOL, f"groupnorm_affine: affine error {float(err):.3e} (bound {AFFINE_TOL} (1 + |y|))"
    return float(err) / AFFINE_TOL


for _kind in ("control", "offset10"):
    case("vae_ops.groupnorm_affine", _kind, "bounded", _gn_affine_check)(lambda dev, k=_kind: _gn_affine(dev, k))


def _gn_from_stats(dev):
    """the statistics a conv epilogue took of its own output (random operands), folded by groupnorm_affine_from_stats"""
    m = Mem(dev)
    T, H, W, cin, cout = 3, 5, 7, 64, 64
    x = U((T * H * W, cin), "dp.gnst.x", math.sqrt(3.0)).to(F16)
    w = U((cout, 27, cin), "dp.gnst.w", math.sqrt(3.0 / (27 * cin))).to(F16)
    b = (3.0 * U((cout,), "dp.gnst.b")).to(F16)
    out, st = (real_fn if str(dev) != "cpu" else double_fn)("vae_ops.conv3d_causal")(x.to(dev), w.to(dev), b.to(dev), T, H, W, cin, cout, gn_stats=True)
    gw, gb = gn_weights(cout, "gnst")
    return Call((st, m.vec("weight", gw), m.vec("bias", gb)), {}, m.watch, ref=(_cpu(out), gw, gb))


case("vae_ops.groupnorm_affine_from_stats", "conv-epilogue-statistics", "bounded", _gn_affine_check)(_gn_from_stats)


def _gn_apply_silu(dev):
    m = Mem(dev)
    x = gn_x(37, 64, "control", "dp.gnap")
    aff = torch.stack([1.0 + U((64,), "dp.gnap.sc", 0.5), U((64,), "dp.gnap.sh")], 1).float().contiguous()
    o = m.out("out", 37, 64, F16, c0=8)
    return Call((m.rows("x", x, pad=8), m.plain("affine", aff), True), {"out": o}, m.watch, {0: o}, (x, aff))


case("vae_ops.groupnorm_apply", "silu", "bounded",
     lambda call, flat, d, peer, is_double: RB.check(_out0(flat), *RB.gn_apply_ref(*call.ref, True), "groupnorm_apply silu"))(_gn_apply_silu)


def _cout4_affine(dev):
    from hunyuanvideo_efficiency_amd import vae_ops
    m = Mem(dev)
    T, H, W, cin, cout = 3, 5, 7, 64, 3
    x, aff, w, b = CB.cout4_operands(T * H * W, cin, cout, CB.cout4_key(T, H, W, cin, cout))
    o = m.out("out", T * H * W, 8, F16, pad=8)
    return Call((m.rows("x", x, pad=8), m.plain("affine", aff), True, m.plain("w_frag", vae_ops.cout4_weight_fragments(w)), m.vec("bias", b),
                 T, H, W, cin, cout), {"out": o}, m.watch, {0: o}, (x, aff, w, b, T, H, W, cout))


def _cout4_check(call, flat, derived, peer, is_double):
    x, aff, w, b, T, H, W, cout = call.ref
    h, au, share = CB.cout4_act(x, aff, True)
    assert share <= CB.AMBIGUOUS_SHARE_LIMIT
    y64, bound = CB.cout4_ref(h, au, w, b, T, H, W)
    got = _out0(flat)
    assert not bool(got[:, cout:].any()), "conv_cout4: columns cout..7 are not zero"
    return RB.check(got[:, :cout], y64, bound, "conv_cout4 affine + SiLU")


case("vae_ops.conv_cout4", "affine+silu", "bounded", _cout4_check)(_cout4_affine)


def _softmax_random(dev, cls, causal):
    m = Mem(dev)
    rows, cols, cols_pad = 24, 21, 24
    s = RB.softmax_scores(cls, rows, cols_pad, "dp.softmax")
    o = m.out("out", rows, cols_pad, F16, c0=8)
    cb = 7 if causal else 0
    return Call((m.rows("S", s, pad=8), cols, cols_pad, 0.125), {"out": o, "causal_block": cb}, m.watch, {0: o},
                (s[:, :cols_pad], RB.valid_of(rows, cols, cb), 0.125))


case("vae_ops.softmax_rows", "spread", "bounded",
     lambda call, flat, d, peer, is_double: RB.check(_out0(flat), *RB.softmax_ref(*call.ref), "softmax_rows"))(lambda dev: _softmax_random(dev, "spread", False))
case("vae_ops.softmax_rows", "peaked-causal", "bounded",
     lambda call, flat, d, peer, is_double: RB.check(_out0(flat), *RB.softmax_ref(*call.ref), "softmax_rows causal"))(lambda dev: _softmax_random(dev, "peaked", True))


ATTN_SCALE = 0.2          # a softmax scale that is not the default 128^-0.5: a double that ignores `scale` fails its bound


def _attn_random(dev, space, n_q, n_kv, scale, **extra):
    m = Mem(dev)
    H = 2
    q, k, v = AB.make_case("random", n_q, n_kv, H, f"dp.{n_q}.{n_kv}")
    Q, K, V = _fused(m, q, k, v, H)
    o = m.out("out", n_q, H * 128, BF16, pad=64)
    kw = {} if space == "sp" or scale is None else {"scale": scale}
    return Call((Q, K, V, o, H), dict(kw, **extra), m.watch, {0: o}, (q, k, v, H, kw.get("scale")))


def _attn_check(call, flat, derived, peer, is_double):
    q, k, v, H, scale = call.ref
    return AB.AttnRef(q, k, v, H, scale=scale, rounded_q=not is_double).check_o(_out0(flat), "attn_fwd")


for _nq, _nkv, _sc in ((321, 65, None), (1, 449, None), (321, 449, ATTN_SCALE)):
    case("ops.attn_fwd", f"random-{_nq}x{_nkv}-scale={_sc}", "bounded", _attn_check)(lambda dev, a=(_nq, _nkv, _sc): _attn_random(dev, "ops", *a))
case("ops.attn_fwd", "random-321x449-no-split-workspace", "bounded", _attn_check)(
    lambda dev: _attn_random(dev, "ops", 321, 449, None, kv_split_workspace=False))
case("sp.attn_fwd", "random-321x65", "bounded", _attn_check)(lambda dev: _attn_random(dev, "sp", 321, 65, None))


def _attn_partial_random(dev, space, n_q, n_kv, splits, merge):
    m = Mem(dev)
    H = 2
    q, k, v = AB.make_case("random", n_q, n_kv, H, f"dp.p.{n_q}.{n_kv}")
    Q, K, V = _fused(m, q, k, v, H)
    mk = real_fn if str(dev) != "cpu" else double_fn
    parts = mk("sp.attn_partials")(splits, n_q, H, dev)
    if not merge:
        return Call((Q, K, V, parts, H, splits), {}, m.watch, ref=(q, k, v, H, splits, parts))
    mk(space + ".attn_partial")(Q, K, V, parts, H, splits)
    o = m.out("out", n_q, H * 128, BF16, pad=64)
    return Call((parts, o), {}, m.watch, {0: o}, (q, k, v, H, splits, parts))


def _attn_partial_check(call, flat, derived, peer, is_double):
    q, k, v, H, splits, parts = call.ref
    n_kv = k.shape[0]
    edges = [0, n_kv] if splits == 1 else [0, KD.split_cut(n_kv), n_kv]
    assert parts.used == splits
    return max(AB.AttnRef(q, k[a:b], v[a:b], H, rounded_q=not is_double).check_partial(_cpu(parts.o[s]), _cpu(parts.ml[s]), f"attn_partial slot {s}")
               for s, (a, b) in enumerate(zip(edges[:-1], edges[1:])))


def _attn_merge_check(call, flat, derived, peer, is_double):
    q, k, v, H, splits, parts = call.ref
    cut = KD.split_cut(k.shape[0])
    ref = AB.AttnRef(q, k, v, H, gap=AB.kernel_gap(q, k, H, cuts=(cut,)), rounded_q=not is_double)
    r = ref.check_o(_out0(flat), "attn_merge")
    r2 = float(AB.merge_ratio(_out0(flat), _cpu(parts.o), _cpu(parts.ml)).max())
    assert r2 <= 1.0, f"attn_merge: the merge of its own partials is off by {r2:.3g} x the bound"
    return max(r, r2)


for _space in ("ops", "sp"):
    for _nq, _nkv, _sp in ((321, 65, 1), (1, 129, 2), (321, 191, 2)):
        case(f"{_space}.attn_partial", f"random-{_nq}x{_nkv}-splits{_sp}", "bounded", _attn_partial_check)(
            lambda dev, a=(_space, _nq, _nkv, _sp): _attn_partial_random(dev, *a, False))
    case(f"{_space}.attn_merge", "random-321x191-splits2", "bounded", _attn_merge_check)(
        lambda dev, s=_space: _attn_partial_random(dev, s, 321, 191, 2, True))


def cases_of(cls=None):
    return [c for c in CASES if cls is None or c.cls == cls]


# ------------------------------------------------------------------------------------------------------------ refusals
@dataclass
class Refusal:
    op: str
    name: str
    build: Callable              # device -> Call (watch: the buffers that must keep every bit); the call breaks exactly one rule

    @property
    def error(self):
        """the name of the exception type BOTH sides must raise (REFUSAL_ERRORS below)"""
        return REFUSAL_ERRORS[self.id]

    @property
    def id(self):
        return f"{self.op}:{self.name}"


REFUSALS = []


def refusal(op, name):
    def deco(build):
        REFUSALS.append(Refusal(op, name, build))
        return build
    return deco


def stride2(t):
    """the same shape with an innermost stride of 2: the one rule broken (the cells it names lie inside the operand's poisoned buffer)"""
    return torch.as_strided(t, t.shape, (t.stride(0), 2), t.storage_offset())


def _legal_gemm(m, M=5, N=64, K=64, pad=24, dt=BF16):
    a, w, b = _gemm_exact_operands(N, K, M, "ref.gemm", False, dt)
    return m.rows("a", a, pad=pad), m.rows("w", w, 2, 7, 40), m.vec("bias", b), m.out("out", M, N, dt, c0=8)


def _rg(name, f, op="ops.gemm"):
    def build(dev):
        m = Mem(dev)
        args, kw = f(m)
        return Call(args, kw, m.watch)
    REFUSALS.append(Refusal(op, name, build))


def _gemm_ref(mod):
    def f(m):
        A, W, B, o = _legal_gemm(m)
        return mod(m, A, W, B, o)
    return f


_rg("a-wrong-dtype", _gemm_ref(lambda m, A, W, B, o: ((A.view(F16), W, B), {"out": o})))
_rg("w-inner-stride-2", _gemm_ref(lambda m, A, W, B, o: ((A, stride2(W), B), {"out": o})))
_rg("a-rows-not-uniform", _gemm_ref(lambda m, A, W, B, o: ((torch.as_strided(A, (2, 2, 64), (3 * A.stride(0), A.stride(0), 1), A.storage_offset()), W, B), {})))
_rg("bias-not-contiguous", _gemm_ref(lambda m, A, W, B, o: ((A, W[:32], B[::2]), {"out": o[:, :32]})))
_rg("n_split-not-multiple-of-8", _gemm_ref(lambda m, A, W, B, o: ((A, W, B), {"out": o, "n_split": 12, "out1": m.out("out1", 5, 64, BF16)})))
_rg("out-rows-disagree", _gemm_ref(lambda m, A, W, B, o: ((A, W, B), {"out": o[:4]})))
_rg("gate-without-res", _gemm_ref(lambda m, A, W, B, o: ((A, W, B), {"out": o, "gate": B})))
_rg("K-not-multiple-of-64", _gemm_ref(lambda m, A, W, B, o: ((A[:, :32], W[:, :32], B), {"out": o})))


def _r_lda(m):
    A, W, B, o = _legal_gemm(m, pad=20)           # row stride 84: not a multiple of 8 elements
    return (A, W, B), {"out": o}


_rg("lda-breaks-16-byte-rule", _r_lda)


def _legal_gemm8(m, K=384, pad=32):
    a, w, b = _gemm_exact_operands(64, K, 5, "ref.gemm8", False, F32)
    return (m.rows("a_q", a.to(FP8), pad=pad), m.vec("a_scale", torch.ones(5)), m.rows("w_q", w.to(FP8), 2, 7, 48),
            m.vec("w_scale", torch.ones(1, dtype=BF16)), m.vec("bias", b.to(BF16)), m.out("out", 5, 64, BF16, c0=8))


def _g8(mod):
    def f(m):
        return mod(m, *_legal_gemm8(m))
    return f


_rg("a_q-wrong-dtype", _g8(lambda m, A, s, W, ws, B, o: ((A.float().to(BF16), s, W, ws, B), {"out": o})), "ops.gemm_fp8")
_rg("K-below-384", _g8(lambda m, A, s, W, ws, B, o: ((A[:, :256], s, W[:, :256], ws, B), {"out": o})), "ops.gemm_fp8")
_rg("a_scale-shorter-than-m", _g8(lambda m, A, s, W, ws, B, o: ((A, s[:3], W, ws, B), {"out": o})), "ops.gemm_fp8")


def _r_lda8(m):
    A, s, W, ws, B, o = _legal_gemm8(m, pad=24)           # 408 bytes per row: a multiple of 8, not of 16
    return (A, s, W, ws, B), {"out": o}


_rg("lda-not-multiple-of-16", _r_lda8, "ops.gemm_fp8")


def _legal_ln(m, D=512, pad=24, opad=16):
    x = RB.data_rows("control", 5, D, "ref.ln")
    sh, sc = _ln_operands(D, "shift+scale", "ref.ln")
    return m.rows("x", x, pad=pad), m.vec("shift", sh), m.vec("scale", sc), m.out("out", 5, D, BF16, pad=opad)


_rg("shift-not-a-[d]-vector", lambda m: (lambda X, sh, sc, o: ((X, sh[:256], sc), {"out": o}))(*_legal_ln(m)), "ops.ln_modulate")
_rg("shift-wrong-dtype", lambda m: (lambda X, sh, sc, o: ((X, sh.float(), sc), {"out": o}))(*_legal_ln(m)), "ops.ln_modulate")
_rg("x-wrong-dtype", lambda m: (lambda X, sh, sc, o: ((X.view(F16), sh, sc), {"out": o}))(*_legal_ln(m)), "ops.ln_modulate")
_rg("x-inner-stride-2", lambda m: (lambda X, sh, sc, o: ((stride2(X), sh, sc), {"out": o}))(*_legal_ln(m)), "ops.ln_modulate")
_rg("ldx-breaks-16-byte-rule", lambda m: (lambda X, sh, sc, o: ((X, sh, sc), {"out": o}))(*_legal_ln(m, pad=12)), "ops.ln_modulate")
_rg("ldo-breaks-16-byte-rule", lambda m: (lambda X, sh, sc, o: ((X, sh, sc), {"out": o}))(*_legal_ln(m, opad=4)), "ops.ln_modulate")
_rg("D-not-multiple-of-8", lambda m: (lambda X, sh, sc, o: ((X[:, :12], sh[:12], sc[:12]), {"out": o[:, :12]}))(*_legal_ln(m)), "ops.ln_modulate")
_rg("out-shape-disagrees", lambda m: (lambda X, sh, sc, o: ((X, sh, sc), {"out": o[:4]}))(*_legal_ln(m)), "ops.ln_modulate")


def _legal_ln8(m, ldq=544):
    X, sh, sc, _ = _legal_ln(m)
    return X, sh, sc, m.bytes("out_q", 5, 512, ldq), m.flat("out_scale", 5, F32)


_rg("ldq-not-multiple-of-16", lambda m: (lambda X, sh, sc, q, s: ((X, sh, sc), {"out_q": q, "out_scale": s}))(*_legal_ln8(m, 520)), "ops.ln_modulate_fp8")
_rg("out_scale-shorter-than-m", lambda m: (lambda X, sh, sc, q, s: ((X, sh, sc), {"out_q": q, "out_scale": s[:4]}))(*_legal_ln8(m)), "ops.ln_modulate_fp8")
_rg("scale-not-contiguous", lambda m: (lambda X, sh, sc, q, s: ((X[:, :256], sh[:256], sc[::2]), {"out_q": q[:, :256], "out_scale": s}))(*_legal_ln8(m)),
    "ops.ln_modulate_fp8")
_rg("x-wrong-dtype", lambda m: (lambda X, sh, sc, q, s: ((X.view(F16),), {"out_q": q, "out_scale": s}))(*_legal_ln8(m)), "ops.quant_rows_fp8")
_rg("out_q-wrong-dtype", lambda m: (lambda X, sh, sc, q, s: ((X,), {"out_q": q.view(torch.uint8), "out_scale": s}))(*_legal_ln8(m)), "ops.quant_rows_fp8")
_rg("ldq-not-multiple-of-16", lambda m: (lambda X, sh, sc, q, s: ((X,), {"out_q": q, "out_scale": s}))(*_legal_ln8(m, 520)), "ops.quant_rows_fp8")


def _legal_qk(m, H=2, n_rows=5, extra=40):
    row, x, w, qw, kw = RB.qk_case("control", H, n_rows, "ref.qk")
    cos, sin = RB.rope_tables_independent(n_rows, "ref.qk")
    return m.rows("qkv", row[:, :3 * H * 128 + extra].clone()), m.vec("q_weight", qw), m.vec("k_weight", kw), m.plain("cos", cos), m.plain("sin", sin), H


_rg("cos-shorter-than-n_rope", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c[:3], s, 4, H, H * 128), {}))(*_legal_qk(m)), "ops.qknorm_rope_")
_rg("cos-wrong-dtype", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c.double(), s, 4, H, H * 128), {}))(*_legal_qk(m)), "ops.qknorm_rope_")
_rg("k_offset-breaks-8-element-rule", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c, s, 4, H, H * 128 + 4), {}))(*_legal_qk(m)), "ops.qknorm_rope_")
_rg("k-heads-overlap-q", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c, s, 4, H, H * 128 - 128), {}))(*_legal_qk(m)), "ops.qknorm_rope_")
_rg("ld-breaks-16-byte-rule", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c, s, 4, H, H * 128), {}))(*_legal_qk(m, extra=44)), "ops.qknorm_rope_")
_rg("qkv-rows-not-uniform", lambda m: (lambda Q, qw, kw, c, s, H: ((torch.as_strided(Q, (2, 2, Q.shape[1]), (3 * Q.stride(0), Q.stride(0), 1), Q.storage_offset()),
                                                                     qw, kw, c, s, 4, H, H * 128), {}))(*_legal_qk(m)), "ops.qknorm_rope_")
_rg("scatter-block-not-whole-heads", lambda m: (lambda Q, qw, kw, c, s, H: ((Q, qw, kw, c, s, 4, H, H * 128),
                                                                             {"out": m.out("out", 5 * 8, 64, BF16, pad=0).view(5, 8, 64)}))(*_legal_qk(m)), "ops.qknorm_rope_")


def _legal_attn(m, pad=24):
    H = 2
    q, k, v = AB.make_case("random", 5, 65, H, "ref.attn")
    return m.rows("q", q, pad=pad), m.rows("k", k), m.rows("v", v), m.out("out", 5, H * 128, BF16, pad=64), H


_rg("row-counts-disagree", lambda m: (lambda Q, K, V, o, H: ((Q, K, V[:64], o, H), {}))(*_legal_attn(m)), "ops.attn_fwd")
_rg("out-rows-disagree", lambda m: (lambda Q, K, V, o, H: ((Q, K, V, o[:4], H), {}))(*_legal_attn(m)), "ops.attn_fwd")
_rg("q-not-2-D", lambda m: (lambda Q, K, V, o, H: ((Q.view(5, H, 128), K, V, o, H), {}))(*_legal_attn(m, pad=0)), "ops.attn_fwd")
_rg("k-wrong-dtype", lambda m: (lambda Q, K, V, o, H: ((Q, K.view(F16), V, o, H), {}))(*_legal_attn(m)), "ops.attn_fwd")
_rg("q-stride-breaks-16-byte-rule", lambda m: (lambda Q, K, V, o, H: ((Q, K, V, o, H), {}))(*_legal_attn(m, pad=12)), "ops.attn_fwd")
_rg("v-inner-stride-2", lambda m: (lambda Q, K, V, o, H: ((Q, K, stride2(V), o, H), {}))(*_legal_attn(m)),
    "ops.attn_fwd")


def _legal_copy3d(m):
    return m.rows("src", special_16((10, 40), "ref.copy3d", BF16), pad=8), m.out("dst", 14, 24, BF16, c0=8, pad=8)


_rg("cols-not-multiple-of-8", lambda m: (lambda s, d: ((s, d, 2, 3, 12, 240, 48, 280, 40), {}))(*_legal_copy3d(m)), "ops.copy3d")
_rg("dst_ld-below-cols", lambda m: (lambda s, d: ((s, d, 2, 3, 24, 240, 48, 280, 16), {}))(*_legal_copy3d(m)), "ops.copy3d")
_rg("src_ld-breaks-8-element-rule", lambda m: (lambda s, d: ((s, d, 2, 3, 24, 240, 44, 280, 40), {}))(*_legal_copy3d(m)), "ops.copy3d")
_rg("src-wrong-dtype", lambda m: (lambda s, d: ((s.view(F16), d, 2, 3, 24, 240, 48, 280, 40), {}))(*_legal_copy3d(m)), "ops.copy3d")
_rg("cols-not-multiple-of-8", lambda m: (lambda s, d: ((s, d, 2, 3, 12, 240, 48, 280, 40), {}))(*_legal_copy3d(m)), "sp.copy3d")


def _legal_gemm_f16(m):
    return _legal_gemm(m, K=128, dt=F16)


_rg("K-not-multiple-of-64", lambda m: (lambda A, W, B, o: ((A, W, B), {"out": o, "k": 96}))(*_legal_gemm_f16(m)), "vae_ops.gemm_f16")
_rg("a-wrong-dtype", lambda m: (lambda A, W, B, o: ((A.view(BF16), W, B), {"out": o}))(*_legal_gemm_f16(m)), "vae_ops.gemm_f16")
_rg("out_f32-with-res", lambda m: (lambda A, W, B, o: ((A, W, B), {"out": m.out("o32", 5, 64, F32), "out_f32": True, "res": o}))(*_legal_gemm_f16(m)),
    "vae_ops.gemm_f16")
_rg("out-dtype-disagrees-with-out_f32", lambda m: (lambda A, W, B, o: ((A, W, B), {"out": o, "out_f32": True}))(*_legal_gemm_f16(m)), "vae_ops.gemm_f16")
_rg("n-not-multiple-of-8", lambda m: (lambda A, W, B, o: ((A, W, B), {"out": o, "n": 12}))(*_legal_gemm_f16(m)), "vae_ops.gemm_f16")


def _legal_conv(m, T=3, H=4, W=6):
    x, w, b = _conv_operands(T * H * W, 64, 64, "ref.conv", False)
    return m.rows("x", x, pad=8), m.plain("w_taps", w), m.vec("bias", b), m.out("out", 4 * H * W, 64, F16, c0=8), H, W


_rg("up_t-with-even-T", lambda m: (lambda X, Wt, B, o, H, W: ((X, Wt, B, 4, H, W, 64, 64), {"up_t": True, "out": o}))(*_legal_conv(m)), "vae_ops.conv3d_causal")
_rg("up_hw-with-odd-W", lambda m: (lambda X, Wt, B, o, H, W: ((X, Wt, B, 3, H, 5, 64, 64), {"up_hw": True, "out": o[:60]}))(*_legal_conv(m)), "vae_ops.conv3d_causal")
_rg("w_taps-size-disagrees", lambda m: (lambda X, Wt, B, o, H, W: ((X, Wt[:32], B, 3, H, W, 64, 64), {"out": o[:72]}))(*_legal_conv(m)), "vae_ops.conv3d_causal")
_rg("x-wrong-dtype", lambda m: (lambda X, Wt, B, o, H, W: ((X.view(BF16), Wt, B, 3, H, W, 64, 64), {"out": o[:72]}))(*_legal_conv(m)), "vae_ops.conv3d_causal")
_rg("cin-not-multiple-of-64", lambda m: (lambda X, Wt, B, o, H, W: ((X, Wt.reshape(-1)[:64 * 27 * 32], B, 3, H, W, 32, 64), {"out": o[:72]}))(*_legal_conv(m)),
    "vae_ops.conv3d_causal")


def _legal_gn_apply(m):
    return (m.rows("x", ints((37, 64), "ref.gnap", 100).to(F16), pad=8), m.plain("affine", torch.ones(64, 2)), m.out("out", 37, 64, F16, c0=8))


_rg("affine-wrong-dtype", lambda m: (lambda x, a, o: ((x, a.to(F16), False), {"out": o}))(*_legal_gn_apply(m)), "vae_ops.groupnorm_apply")
_rg("x-inner-stride-2", lambda m: (lambda x, a, o: ((stride2(x), a, False), {"out": o}))(*_legal_gn_apply(m)), "vae_ops.groupnorm_apply")
_rg("x-wrong-dtype", lambda m: (lambda x, a, o: ((x.view(BF16), a, True), {"out": o}))(*_legal_gn_apply(m)), "vae_ops.groupnorm_apply")


def _legal_softmax(m):
    return m.rows("S", torch.full((8, 16), 4.0), pad=8), m.out("out", 8, 16, F16, c0=8)


_rg("S-wrong-dtype", lambda m: (lambda s, o: ((s.to(F16), 8, 16, 0.5), {"out": o}))(*_legal_softmax(m)), "vae_ops.softmax_rows")
_rg("cols-above-cols_pad", lambda m: (lambda s, o: ((s, 17, 16, 0.5), {"out": o}))(*_legal_softmax(m)), "vae_ops.softmax_rows")
_rg("negative-causal_block", lambda m: (lambda s, o: ((s, 8, 16, 0.5), {"out": o, "causal_block": -1}))(*_legal_softmax(m)), "vae_ops.softmax_rows")
_rg("S-inner-stride-2", lambda m: (lambda s, o: ((stride2(s), 8, 16, 0.5), {"out": o}))(*_legal_softmax(m)), "vae_ops.softmax_rows")



def _legal_cout4(m, c0=0):
    from hunyuanvideo_efficiency_amd import vae_ops
    T, H, W, cin, cout = 1, 2, 3, 64, 3
    w = ints((cout, cin, 3, 3, 3), "ref.c4.w", 1).to(F16)
    return ((m.rows("x", ints((T * H * W, cin), "ref.c4.x").to(F16), pad=8), None, False, m.plain("w_frag", vae_ops.cout4_weight_fragments(w)),
             m.vec("bias", ints((cout,), "ref.c4.b", 9).to(F16)), T, H, W, cin, cout), m.out("out", T * H * W, 8, F16, c0=c0, pad=8 - c0))


_rg("out-column-offset-breaks-16-byte-rule", lambda m: (lambda a, o: (a, {"out": o}))(*_legal_cout4(m, c0=4)), "vae_ops.conv_cout4")
_rg("x-wrong-dtype", lambda m: (lambda a, o: ((a[0].view(BF16),) + a[1:], {"out": o}))(*_legal_cout4(m)), "vae_ops.conv_cout4")
_rg("rows-disagree-with-the-grid", lambda m: (lambda a, o: ((a[0][:5],) + a[1:], {"out": o}))(*_legal_cout4(m)), "vae_ops.conv_cout4")
_rg("x-not-contiguous", lambda m: ((m.rows("x", ints((8, 40), "ref.mm", 9).to(BF16), pad=8), None), {}), "ops.masked_mean")
_rg("mask-wrong-dtype", lambda m: ((m.plain("x", ints((8, 40), "ref.mm", 9).to(BF16)), m.plain("mask", torch.ones(8, dtype=torch.int64))), {}), "ops.masked_mean")


# the rest of the VAE entry points: one refusal each
def _x16(m, rows=6, C=16, dt=F16):
    return m.rows("x", ints((rows, C), "ref.x16", 9).to(dt), pad=8)


_rg("weight-wrong-dtype", lambda m: ((_x16(m, 6, 64), m.vec("weight", torch.ones(64, dtype=F32)), m.vec("bias", torch.zeros(64, dtype=F16))), {}),
    "vae_ops.groupnorm_affine")
_rg("x-wrong-dtype", lambda m: ((_x16(m, dt=BF16), 2, 3, 2, 2), {}), "vae_ops.temporal_avg_pool")
_rg("x-wrong-dtype", lambda m: ((_x16(m, dt=BF16), 2, 3, 2), {}), "vae_ops.temporal_nearest_up")
_rg("x-inner-stride-2", lambda m: ((stride2(_x16(m)), 2, 3, 2), {}), "vae_ops.temporal_linear_up")
_rg("src-not-16-bit", lambda m: ((m.rows("src", torch.ones(6, 8), pad=8), m.out("dst", 8, 6, F16, pad=10)), {}), "vae_ops.transpose_16b")
_rg("z-wrong-dtype", lambda m: ((m.crop("z", finite_f16((5, 2, 3, 4), "ref.z")), 8), {}), "vae_ops.latent_tile")
_rg("cpad-below-C", lambda m: ((m.crop("z", special_f32((5, 2, 3, 4), "ref.z32")), 4), {}), "vae_ops.latent_tile")
_rg("shapes-disagree", lambda m: ((m.crop("src", special_16((3, 2, 3, 5), "ref.c4d", F16)), m.crop("dst", shape=(3, 2, 3, 4), dtype=F16)), {}),
    "vae_ops.copy4d_")


def _r_strided_out(m):
    x, w, b = _conv_operands(2 * 4 * 6, 64, 64, "ref.strided", False)
    return (m.rows("x", x, pad=8), m.plain("w_taps", w), m.vec("bias", b), 2, 4, 6, 64, 64), {"stride": (1, 2, 2), "out": m.out("out", 2 * 4 * 6, 64, F16, c0=8)}


_rg("out-shape-disagrees-with-the-grid", _r_strided_out, "vae_ops.conv3d_causal_strided")


def _r_subpixel_table(m):
    from hunyuanvideo_efficiency_amd import vae_ops
    w_sub, table, ntap = vae_ops.subpixel_weights(ints((136, 256, 3, 3, 3), "ref.subpix.w", 1).to(F16), False)
    return (m.rows("x", ints((1 * 2 * 2, 256), "ref.subpix.x").to(F16), pad=8), m.plain("w_sub", w_sub), m.plain("table", table.long()), ntap,
            m.vec("bias", torch.zeros(136, dtype=F16)), 1, 2, 2, 256, 136, False), {}


_rg("tap-table-wrong-dtype", _r_subpixel_table, "vae_ops.conv3d_upsampled_subpixel")


def _r_from_stats(m):
    st = KD.gn_stats_of(ints((6, 64), "ref.gnst", 9).to(F16))
    st.partial = st.partial.to(m.dev)
    return (st, m.vec("weight", torch.ones(64, dtype=F16)), m.vec("bias", torch.zeros(64, dtype=F32))), {}


_rg("bias-wrong-dtype", _r_from_stats, "vae_ops.groupnorm_affine_from_stats")


# the exception type of the one rule each refusal breaks, as ops.py / vae_ops.py raise it: TypeError and ValueError from _chk / _rows,
# AssertionError from a wrapper's own assert, HVKernelError where the C ABI answers HV_ERR_ARG (or the wrapper raises it itself)
REFUSAL_ERRORS = {
    "ops.gemm:a-wrong-dtype": "TypeError",
    "ops.gemm:w-inner-stride-2": "ValueError",
    "ops.gemm:a-rows-not-uniform": "ValueError",
    "ops.gemm:bias-not-contiguous": "ValueError",
    "ops.gemm:n_split-not-multiple-of-8": "HVKernelError",
    "ops.gemm:out-rows-disagree": "AssertionError",
    "ops.gemm:gate-without-res": "HVKernelError",
    "ops.gemm:K-not-multiple-of-64": "HVKernelError",
    "ops.gemm:lda-breaks-16-byte-rule": "HVKernelError",
    "ops.gemm_fp8:a_q-wrong-dtype": "HVKernelError",
    "ops.gemm_fp8:K-below-384": "HVKernelError",
    "ops.gemm_fp8:a_scale-shorter-than-m": "AssertionError",
    "ops.gemm_fp8:lda-not-multiple-of-16": "HVKernelError",
    "ops.ln_modulate:shift-not-a-[d]-vector": "AssertionError",
    "ops.ln_modulate:shift-wrong-dtype": "TypeError",
    "ops.ln_modulate:x-wrong-dtype": "TypeError",
    "ops.ln_modulate:x-inner-stride-2": "ValueError",
    "ops.ln_modulate:ldx-breaks-16-byte-rule": "HVKernelError",
    "ops.ln_modulate:ldo-breaks-16-byte-rule": "HVKernelError",
    "ops.ln_modulate:D-not-multiple-of-8": "HVKernelError",
    "ops.ln_modulate:out-shape-disagrees": "AssertionError",
    "ops.ln_modulate_fp8:ldq-not-multiple-of-16": "HVKernelError",
    "ops.ln_modulate_fp8:out_scale-shorter-than-m": "AssertionError",
    "ops.ln_modulate_fp8:scale-not-contiguous": "ValueError",
    "ops.quant_rows_fp8:x-wrong-dtype": "TypeError",
    "ops.quant_rows_fp8:out_q-wrong-dtype": "AssertionError",
    "ops.quant_rows_fp8:ldq-not-multiple-of-16": "HVKernelError",
    "ops.qknorm_rope_:cos-shorter-than-n_rope": "AssertionError",
    "ops.qknorm_rope_:cos-wrong-dtype": "TypeError",
    "ops.qknorm_rope_:k_offset-breaks-8-element-rule": "HVKernelError",
    "ops.qknorm_rope_:k-heads-overlap-q": "HVKernelError",
    "ops.qknorm_rope_:ld-breaks-16-byte-rule": "HVKernelError",
    "ops.qknorm_rope_:qkv-rows-not-uniform": "ValueError",
    "ops.qknorm_rope_:scatter-block-not-whole-heads": "AssertionError",
    "ops.attn_fwd:row-counts-disagree": "AssertionError",
    "ops.attn_fwd:out-rows-disagree": "AssertionError",
    "ops.attn_fwd:q-not-2-D": "AssertionError",
    "ops.attn_fwd:k-wrong-dtype": "TypeError",
    "ops.attn_fwd:q-stride-breaks-16-byte-rule": "HVKernelError",
    "ops.attn_fwd:v-inner-stride-2": "ValueError",
    "ops.copy3d:cols-not-multiple-of-8": "HVKernelError",
    "ops.copy3d:dst_ld-below-cols": "HVKernelError",
    "ops.copy3d:src_ld-breaks-8-element-rule": "HVKernelError",
    "ops.copy3d:src-wrong-dtype": "TypeError",
    "sp.copy3d:cols-not-multiple-of-8": "HVKernelError",
    "vae_ops.gemm_f16:K-not-multiple-of-64": "HVKernelError",
    "vae_ops.gemm_f16:a-wrong-dtype": "TypeError",
    "vae_ops.gemm_f16:out_f32-with-res": "HVKernelError",
    "vae_ops.gemm_f16:out-dtype-disagrees-with-out_f32": "TypeError",
    "vae_ops.gemm_f16:n-not-multiple-of-8": "HVKernelError",
    "vae_ops.conv3d_causal:up_t-with-even-T": "HVKernelError",
    "vae_ops.conv3d_causal:up_hw-with-odd-W": "HVKernelError",
    "vae_ops.conv3d_causal:w_taps-size-disagrees": "AssertionError",
    "vae_ops.conv3d_causal:x-wrong-dtype": "TypeError",
    "vae_ops.conv3d_causal:cin-not-multiple-of-64": "HVKernelError",
    "vae_ops.groupnorm_apply:affine-wrong-dtype": "TypeError",
    "vae_ops.groupnorm_apply:x-inner-stride-2": "ValueError",
    "vae_ops.groupnorm_apply:x-wrong-dtype": "TypeError",
    "vae_ops.softmax_rows:S-wrong-dtype": "TypeError",
    "vae_ops.softmax_rows:cols-above-cols_pad": "HVKernelError",
    "vae_ops.softmax_rows:negative-causal_block": "HVKernelError",
    "vae_ops.softmax_rows:S-inner-stride-2": "ValueError",
    "vae_ops.conv_cout4:out-column-offset-breaks-16-byte-rule": "HVKernelError",
    "vae_ops.conv_cout4:x-wrong-dtype": "TypeError",
    "vae_ops.conv_cout4:rows-disagree-with-the-grid": "AssertionError",
    "ops.masked_mean:x-not-contiguous": "AssertionError",
    "ops.masked_mean:mask-wrong-dtype": "TypeError",
    "vae_ops.groupnorm_affine:weight-wrong-dtype": "TypeError",
    "vae_ops.temporal_avg_pool:x-wrong-dtype": "TypeError",
    "vae_ops.temporal_nearest_up:x-wrong-dtype": "TypeError",
    "vae_ops.temporal_linear_up:x-inner-stride-2": "ValueError",
    "vae_ops.transpose_16b:src-not-16-bit": "AssertionError",
    "vae_ops.latent_tile:z-wrong-dtype": "TypeError",
    "vae_ops.latent_tile:cpad-below-C": "HVKernelError",
    "vae_ops.copy4d_:shapes-disagree": "AssertionError",
    "vae_ops.conv3d_causal_strided:out-shape-disagrees-with-the-grid": "AssertionError",
    "vae_ops.conv3d_upsampled_subpixel:tap-table-wrong-dtype": "TypeError",
    "vae_ops.groupnorm_affine_from_stats:bias-wrong-dtype": "TypeError",
}


def check_refusal(fn, ref: Refusal, device, extra_errors=()):
    """the call raises one of the wrappers' errors and no watched cell changes"""
    from hunyuanvideo_efficiency_amd._abi import HVKernelError
    call = ref.build(device)
    before = {k: bits(v) for k, v in call.watch.items()}
    try:
        fn(*call.args, **call.kwargs)
    except (TypeError, ValueError, AssertionError, HVKernelError) + tuple(extra_errors) as e:
        err = e
    else:
        raise ParityError("refusal", f"{ref.id}: the call was accepted")
    if type(err).__name__ != ref.error:
        raise ParityError("refusal", f"{ref.id}: refused with {type(err).__name__} ({err}), the rule it breaks raises {ref.error}")
    if str(device) != "cpu":
        torch.cuda.synchronize()
    for k, v in call.watch.items():
        if not torch.equal(before[k], bits(v)):
            raise ParityError("refusal", f"{ref.id}: refused with {type(err).__name__}, but buffer {k!r} was written")
    return err
