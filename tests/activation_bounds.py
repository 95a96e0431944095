"""fp64 references, per-element error bounds, the specials table and the value sets of the two nonlinearities gelu_tanh_f and silu_f
(csrc/hv_common.hpp), in the conventions of tests/error_bounds.py and tests/rowwise_bounds.py (ulp_out, EPS32 = 2^-24; every reference
is fp64 on the exact 16-bit input values; a bound is one ulp of the output format plus the first-order fp32 error of the kernel's own
operation sequence).  The input of both functions is a 16-bit value at every call site, so the whole domain - 65,536 patterns per
format - is enumerated.  tests/test_activation_bounds_cpu.py shows what the bounds, the specials table and the mismatch caps accept
(faithful fp32 emulations) and reject (the listed ways an activation can be subtly wrong); tests/test_gpu_activation_domain.py runs
every call site over the same sets.

References (finite wherever the true value is):  gelu64(x) = x sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3);  silu64(x) = x sigmoid(x).

Bound of one evaluation for the output type dt:   |got - f64(x)| <= ulp_out(f64, dt) + E32(x) + FLOOR(x).

E32 of gelu_tanh_f, term by term (every fp32 operation rounds by at most 2^-24 relative, v_exp_f32 and v_rcp_f32 by 1 ulp = 2^-23):
    u = k0 (x + k1 x x x)        three products and the constant k1 (4 roundings of the cubic term), the sum (x and the cubic term have
                                 the same sign: no cancellation), the product with k0 and the constant k0: |du| <= 7 * 2^-24 |u|
    a = u * 2.885..              the constant and the product: |da| <= 9 * 2^-24 |a|, an ABSOLUTE error of 9 * 2^-24 |2u| in the
                                 exponent of e = exp(2u): it grows with |u|
    e = exp2(a)                  1 ulp: altogether e (1 + eps_e), |eps_e| <= (18 |u| + 2) 2^-24
    g = x e / (1 + e)            d ln g / d ln e = 1 / (1 + e) = 1 - s, s = sigmoid(2u): relative part (1 - s) (18 |u| + 2) 2^-24 |g|
    1 + t, 0.5 x (1 + t)         the rounding of 1 + t and of the last product (0.5 x is exact): 2 * 2^-24 |g|
    t = 1 - 2 rcp(e + 1)         this is the cancellation.  r = rcp(e + 1) carries the rounding of e + 1 (2^-24) and v_rcp_f32's ulp
                                 (2^-23): |d(2r)| <= 3 * 2^-24 * 2r, 2r = 2 (1 - s); the subtraction (or the FMA it contracts to) rounds
                                 by 2^-24 |t|, t = tanh u.  These are ABSOLUTE errors of 1 + t = 2s:
                                     delta(x) = (6 (1 - s) + |tanh u|) 2^-24  <=  DELTA = 7 * 2^-24  (= 1.75 * 2^-22),
                                 reached in the negative tail (s -> 0), where 1 + t itself is smaller than delta and the result is
                                 delta's worth of noise times x / 2: the absolute part |x| delta(x) / 2.
    E32_gelu(x) = |g| ((1 - s) (18 |u| + 2) + 2) 2^-24 + |x| delta(x) / 2.
Outside the tail the absolute part is far below the output ulp (at x = 1: 2^-24 against a bf16 ulp of 2^-7 |g|) and the usual "within
one ulp" holds; in x < -4 (bf16; -3.5 for fp16) it exceeds the output ulp of the true value, which decays like exp(-x^2): there the
contract is the absolute error |x| delta / 2 (below |x| 2^-22: nothing a model can see), and torch's own fp32 gelu shares it.

E32 of silu_f: rowwise_bounds.silu_e32, derived in rowwise_bounds.gn_apply_ref: |y| ((|x| + 2) 2^-24 + 2^-22).  Purely relative: SiLU
has no cancellation, its only departure from "exact" is the overflow below.

FLOOR(x), the absolute term for values the fp32 pipeline may flush.  It is not one constant for the whole domain: it is zero wherever
nothing can be flushed, so that it cannot hide a wrong normal result there.
    FLUSH = 2^-126 where |x| < 2^-124: the input, the products u and a, or the result x / 2 is below the smallest normal fp32 (2^-126) and
            a unit that does not keep subnormals (v_exp_f32 and v_rcp_f32 never do; an MFMA or a conversion may not) returns 0 for it.
            Both functions have slope <= 1.13, the flushed quantity is below 2^-126 in the result's units: FLUSH covers it.
    FLOOR = 128 * 2^-126 where x <= -87.33 (SiLU only): from there on 1 + exp(-x) >= 2^126, its reciprocal is below the smallest normal
            fp32 and v_rcp_f32 may return 0; below x = -88.72 exp2's argument passes 128, __expf returns inf and the result is -0 on
            any hardware.  The true value there is |x| exp(x) <= 87.4 * 2^-126 (decreasing with |x|), a NORMAL bf16 number for
            x > -91.9, so no floor below the smallest normal bf16 can accept the shipped formula; 128 * 2^-126 = 2^-119 is the next
            power of two above 87.4 * 2^-126.  It is one bf16 ulp at 2^-112: nothing of that size is ever hidden outside this region.
    GELU needs no FLOOR in its tail: a flushed e gives 1 + t = 0 exactly, which the absolute part |x| delta / 2 (>= 2 * 2^-22) covers.

Specials (SPECIALS; the values are those of torch's fp32 F.gelu(approximate="tanh") and F.silu on the CPU, which is what the reference
model runs - the CPU test asserts that): +inf -> +inf; -inf -> NaN (0.5 * -inf * (1 + -1) and -inf * rcp(inf) are both inf * 0: torch
and the shipped formula agree on NaN); NaN -> NaN; -0 -> -0; +0 -> +0.  A site that accumulates (a GEMM, whose fp32 accumulator starts at
+0) can never hold -0 as a pre-activation: +0 + -0 = +0; such a site is checked with accumulates=True (both zeros give +0).

Value sets: all_bf16(), all_fp16() in bit order; offset_set(dt): fp32 pre-activations v +- 1/4, 3/8, 1/2 ulp(v) with the two 16-bit
addends (v, d) that produce them exactly in an fp32 accumulator.  The contract result is act(RNE_dt(v + d)), known exactly; an activation
applied to the unrounded sum, or to a truncated one, differs from it in bits on a large share of the set.  v runs over every finite
normal value of dt whose addend 1/8 ulp(v) can be written in dt (bf16: a normal number, since the addend passes through an MFMA that
may flush: |v| >= 2^-116; fp16: any number, |v| >= 2^-11 - below that the offsets cannot be written as a 16-bit addend at all), and an
offset that rounds past the largest finite value is left out.

Exactness (mismatch_share, rowwise_bounds' convention): the share of elements whose BITS differ from round-to-nearest-even of the fp64
reference; the cap is 4 x the largest share a faithful fp32 emulation reaches, never below 2 / numel.  Three classes per function and dtype:
    exact    all finite inputs (the tail, the flushed ends and the SiLU overflow included: this share mostly counts those)
    core     the finite inputs with E32 + FLOOR <= ulp / 16: outside the tails, where a faithful kernel misses only next to a rounding tie
    offset   the offset set, inside offset_window()
Measured by tests/test_activation_bounds_cpu.py::test_measured_shares (the kernel's formula in fp32 with exp2 and rcp exact and each
moved by +-1 ulp, with flushing units, and torch's own fp32 functions; the run prints them), largest share and the emulation reaching it:

    gelu bf16   exact 0.2483  (exp2 - 1 ulp, rcp + 1 ulp)   core 0.00003   offset 0.00042 (torch's fp32 gelu)
    gelu fp16   exact 0.2302  (exp2 + 1 ulp, rcp - 1 ulp)   core 0.00036   offset 0.00067
    silu bf16   exact 0.0081  (everything flushed)          core 0.00007   offset 0.00075
    silu fp16   exact 0.00014                               core 0.00015   offset 0.00024

GELU's exact class says nothing (cap 1): a reciprocal that is one ulp high at rcp(1) = 1 makes 1 + t = -2^-22 for EVERY x below the tail,
a quarter of all inputs, and the bound |x| delta / 2 has to accept that.  With exact exp2 and rcp the formula differs from RNE(fp64) on
169 of the 65,280 finite bf16 inputs (168 inside tail_mask, x <= -3.19) and on 500 of the 63,488 fp16 inputs (494 inside, x <= -2.49); SiLU
on 17 (all below -88.7) and on 1.  The core and offset classes carry the check.
The offset share is taken inside offset_window() - where the functions are curved and outside GELU's tail.

The mutants that skip or truncate the pre-rounding reach 0.36 .. 0.51 there (same file)."""
from __future__ import annotations

import math

import torch

from tests.error_bounds import EPS32, ulp_out  # noqa: F401
from tests.rowwise_bounds import check, mismatch_share, ratio, silu_e32  # noqa: F401

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
K0, K1 = math.sqrt(2.0 / math.pi), 0.044715
DELTA = 7.0 * EPS32                  # the largest absolute error of 1 + t (derived above)
FLUSH = 2.0 ** -126                  # one flushed fp32 subnormal
FLOOR = 128.0 * 2.0 ** -126          # SiLU where rcp's result is subnormal or __expf has overflowed
SILU_FLOOR_FROM = -87.33             # 1 + exp(-x) >= 2^126 from here down
NAME = {BF16: "bf16", F16: "fp16"}

# largest mismatch share of a faithful fp32 emulation per function, dtype and class (test_activation_bounds_cpu.py::test_measured_shares
# measures them and fails if one is exceeded or stale)
MEASURED_SHARE = {
    "gelu.bf16.exact": 0.2483, "gelu.bf16.core": 0.00003, "gelu.bf16.offset": 0.00042,
    "gelu.fp16.exact": 0.2302, "gelu.fp16.core": 0.00036, "gelu.fp16.offset": 0.00067,
    "silu.bf16.exact": 0.0081, "silu.bf16.core": 0.00007, "silu.bf16.offset": 0.00075,
    "silu.fp16.exact": 0.00014, "silu.fp16.core": 0.00015, "silu.fp16.offset": 0.00024,
}


def mismatch_cap(fn: str, dtype, cls: str, numel: int) -> float:
    return max(4.0 * MEASURED_SHARE[f"{fn}.{NAME[dtype]}.{cls}"], 2.0 / max(numel, 1))


# ---------------------------------------------------------------------------------------------------- references
def gelu64(x):
    x64 = x.double()
    return x64 * torch.sigmoid(2.0 * K0 * (x64 + K1 * x64 ** 3))


def silu64(x):
    x64 = x.double()
    return x64 * torch.sigmoid(x64)


ACT64 = {"gelu": gelu64, "silu": silu64}


def gelu_parts(x):
    """(g64, relative part, absolute part) of E32_gelu; the absolute part is what the tail is made of"""
    x64 = x.double()
    u = K0 * (x64 + K1 * x64 ** 3)
    s = torch.sigmoid(2.0 * u)
    g = x64 * s
    delta = (6.0 * (1.0 - s) + torch.tanh(u).abs()) * EPS32
    rel = g.abs() * ((1.0 - s) * (18.0 * u.abs() + 2.0) + 2.0) * EPS32
    rel = torch.where(torch.isfinite(rel), rel, torch.zeros_like(rel))       # (1 - s) |u| = 0 * inf for a huge positive x: the term is 0
    return g, rel, 0.5 * x64.abs() * delta


def floor_term(fn: str, x):
    x64 = x.double()
    f = torch.where(x64.abs() < 2.0 ** -124, torch.full_like(x64, FLUSH), torch.zeros_like(x64))
    if fn == "silu":
        f = torch.where(x64 <= SILU_FLOOR_FROM, torch.full_like(x64, FLOOR), f)
    return f


def act_ref(fn: str, x, dtype):
    """(y64, e32, bound) for finite x: e32 = E32 + FLOOR, bound = ulp_out(y64, dtype) + e32"""
    if fn == "gelu":
        y, rel, ab = gelu_parts(x)
        e32 = rel + ab
    else:
        y = silu64(x)
        e32 = silu_e32(x.double(), y)
    e32 = e32 + floor_term(fn, x)
    return y, e32, ulp_out(y, dtype) + e32


def core_mask(y64, e32, dtype):
    return e32 <= ulp_out(y64, dtype) / 16.0


def tail_mask(fn: str, x, dtype):
    """where the absolute part of E32_gelu exceeds a sixteenth of the output ulp (empty for SiLU)"""
    if fn != "gelu":
        return torch.zeros(x.shape, dtype=torch.bool, device=x.device)
    y, _, ab = gelu_parts(x)
    return ab > ulp_out(y, dtype) / 16.0


# ---------------------------------------------------------------------------------------------------- specials
# (input, expected): the fp32 results of torch's F.gelu(approximate="tanh") and F.silu on the CPU; -inf gives NaN in torch and in the
# shipped formulas alike (inf * 0)
SPECIALS = [(math.inf, math.inf), (-math.inf, math.nan), (math.nan, math.nan), (-0.0, -0.0), (0.0, 0.0)]


def specials_violations(got, x, accumulates: bool = False):
    """the indices at which `got` breaks the specials table for the inputs x (same shape, any float dtype): +inf -> +inf, -inf -> NaN,
    NaN -> NaN (every NaN pattern), a zero keeps its sign (accumulates: both zeros give +0, see the module docstring)"""
    g, xx = got.float().reshape(-1), x.float().reshape(-1).to(got.device)
    bad = torch.zeros_like(g, dtype=torch.bool)
    bad |= (xx == math.inf) & ~(g == math.inf)
    bad |= ((xx == -math.inf) | torch.isnan(xx)) & ~torch.isnan(g)
    zero = xx == 0
    neg_in = torch.signbit(xx) & (not accumulates)
    bad |= zero & ~((g == 0) & (torch.signbit(g) == neg_in))
    return bad.nonzero().reshape(-1)


# ---------------------------------------------------------------------------------------------------- value sets
def all_bf16():
    """every bf16 bit pattern, in bit order"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)


def all_fp16():
    """every fp16 bit pattern, in bit order (metrics_bounds.fp16_all, as a torch tensor)"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(F16)


def all_values(dtype):
    return all_bf16() if dtype == BF16 else all_fp16()


def finite_values(dtype):
    v = all_values(dtype)
    return v[torch.isfinite(v.float())]


OFFSETS = [s * f for f in (0.25, 0.375, 0.5) for s in (1.0, -1.0)]      # in ulp(v); 1/2 is the rounding tie


def offset_set(dtype):
    """(v, d, pre32): 16-bit addends v and d, and pre32 = v + d in fp32 (exact: v + d needs 11 more bits than v's leading one at most) =
    v +- 1/4, 3/8, 1/2 ulp(v) for every v described in the module docstring, ordered offset-major (all v at +1/4, all v at -1/4, ...)"""
    mant = 7 if dtype == BF16 else 10
    v = finite_values(dtype)
    tiny = torch.finfo(dtype).tiny
    least = tiny if dtype == BF16 else 2.0 ** -24          # the smallest addend: a normal bf16 (it passes through an MFMA), any fp16
    a = v.double().abs()
    e = torch.floor(torch.log2(a.clamp(min=tiny)))
    ulp = torch.exp2(e - mant)
    ok = (a >= tiny) & (ulp / 8.0 >= least)
    v, ulp = v[ok], ulp[ok]
    vs, ds = [], []
    for off in OFFSETS:
        d = (off * ulp).to(dtype)
        assert bool((d.double() == off * ulp).all())
        keep = torch.isfinite((v.double() + d.double()).to(dtype).float())
        vs.append(v[keep]), ds.append(d[keep])
    v, d = torch.cat(vs), torch.cat(ds)
    pre32 = v.float() + d.float()
    assert bool((pre32.double() == v.double() + d.double()).all())
    return v, d, pre32


def offset_window(v, y64, e32, dtype):
    """the part of the offset set on which its mismatch share is taken: 2^-4 <= |v| < 8, where both functions are curved, less GELU's
    tail (core_mask: there a faithful kernel differs from the fp64 value anyway).  Over most
    binades they are linear (x / 2 near zero; x, or 0, far out), and there rounding the fp32 result at the store reproduces the skipped
    pre-rounding bit for bit: over the whole set a kernel that skips it differs on 3 % of the elements, inside the window on 20 % and more"""
    a = v.double().abs()
    return (a >= 2.0 ** -4) & (a < 8.0) & core_mask(y64, e32, dtype)


def rne(pre, dtype):
    """the contract's pre-rounding: round to nearest even into dtype (torch's conversion from fp32)"""
    return pre.float().to(dtype)
