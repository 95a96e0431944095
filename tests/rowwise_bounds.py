"""fp64 references and per-element error bounds of the row-wise kernels (csrc/hv_rowwise.hip) and of the streaming half of
csrc/hv_vae.hip, in the conventions of tests/error_bounds.py (ulp_out, EPS32 = 2^-24, C = 4; every reference is fp64 on the exact
16-bit input values; a bound is one ulp of the output format plus the first-order fp32 error of the kernel's own operation sequence).
Each derivation stands next to its bound.  tests/test_rowwise_bounds_cpu.py shows what the bounds accept (faithful fp32 emulations in
several summation orders) and what they reject (the listed ways such a kernel can be subtly wrong).

Exactness of the contract roundings (mismatch_share).  A one-ulp bound cannot see a skipped intermediate rounding - bf16(1 + scale) of
the LayerNorm, the cast before the RMSNorm gain, the single rounding of the RoPE expression, SiLU(x) rounded to bf16 in front of the
small-M linear - because it moves a result by half an ulp.  mismatch_share is the share of unambiguous elements whose BITS differ from
round-to-nearest-even of the fp64 reference; a faithful fp32 kernel differs only where its fp32 error carries a value across a rounding
tie.  Measured on the CPU (test_mismatch_share_of_faithful_emulations: every data class and shape of the GPU tests, three summation
orders), the largest share a faithful emulation reaches and the cap = 4 x that (never below 2 / numel; the factor 4 covers a summation
order unluckier than the sampled ones):

    LayerNorm + modulate, control rows    largest 0.0008 (D = 504, affine)                   cap 0.0032
                          offset rows     largest 0.159  (D = 504, no shift, no scale)         cap 0.64
                          massive rows    largest 0.125  (D = 1000, scale only)                cap 0.50
                          constant rows   largest 0 (the output is the shift, exactly)         cap 2 / numel
    RMSNorm + gain + RoPE                 largest 0.0001                                       cap 0.0004
    small-M linear, silu_in               largest 0 (of 164 outputs per case)                  cap 2 / numel

The LayerNorm cap is kept per data class, which is never looser than one cap over all classes: bf16 holds 500 +- 1 as 498, 500, 502, so
an offset row (two of the five massive rows are such rows) has three distinct outputs per row and modulation value, and a single one of
them near a rounding tie moves a sixth of the row at once - the share says little there, and one cap over all classes (0.64) would
say nothing on the control rows, where a skipped rounding is to be seen.

The mutants that skip a rounding reach 0.2 .. 0.5 (same test)."""
from __future__ import annotations

import math
from typing import Optional

import torch

from tests.error_bounds import C, EPS32, Ref, gemm_ref, ulp_out  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

# largest mismatch share of a faithful fp32 emulation (tests/test_rowwise_bounds_cpu.py measures them and fails if one is exceeded)
MEASURED_SHARE = {"ln.control": 0.0008, "ln.offset": 0.159, "ln.massive": 0.125, "ln.constant": 0.0, "qknorm": 0.0001, "silu_in": 0.0}


def mismatch_cap(op: str, numel: int) -> float:
    return max(4.0 * MEASURED_SHARE[op], 2.0 / numel)


def mismatch_share(got: torch.Tensor, y64: torch.Tensor, dtype, ambiguous: Optional[torch.Tensor] = None) -> float:
    """share of the unambiguous elements of `got` whose bits differ from round-to-nearest-even of y64 (+-0 count as equal)"""
    want = y64.to(dtype)
    diff = (got.to(y64.device) != want) | ~torch.isfinite(got.to(y64.device).double())
    if ambiguous is not None:
        diff = diff & ~ambiguous
        n = int((~ambiguous).sum())
    else:
        n = diff.numel()
    return float(diff.sum()) / max(n, 1)


def ratio(got: torch.Tensor, y64: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    g = got.double().to(y64.device)
    r = (g - y64).abs() / bound
    return torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))


def check(got, y64, bound, what: str = "", skip: Optional[torch.Tensor] = None) -> float:
    """asserts every element (outside `skip`) within its bound; names rows and columns as error_bounds.check does; returns the largest
    error-to-bound ratio"""
    r = ratio(got, y64, bound)
    if skip is not None:
        r = torch.where(skip, torch.zeros_like(r), r)
    r2 = r.reshape(-1, r.shape[-1]) if r.dim() > 1 else r.reshape(1, -1)
    worst = float(r2.max()) if r2.numel() else 0.0
    if not worst <= 1.0:
        bad = (r2 > 1.0).nonzero()
        i = int(r2.reshape(-1).argmax())
        m, n = divmod(i, r2.shape[1])
        rows, cols = bad[:, 0], bad[:, 1]
        raise AssertionError(f"{what}: {bad.shape[0]} of {r2.numel()} elements outside the fp64 error bound (worst ratio {worst:.3g} at "
                             f"[{m}, {n}]: got {float(got.reshape(-1)[i])}, y64 {float(y64.reshape(-1)[i]):.9g}); rows "
                             f"[{int(rows.min())}, {int(rows.max())}], cols [{int(cols.min())}, {int(cols.max())}]")
    return worst


# ---------------------------------------------------------------------------------------------------- LayerNorm + modulate / affine
def ln_ref(x, add=None, mul=None, eps: float = 1e-6, affine: bool = False):
    """y64 = z m + a, z = (x - mean) / sqrt(var + eps) in fp64 (two passes); m = bf16(1 + scale) formed as the kernel forms it (fp32
    add, one rounding to bf16 - the same two IEEE operations in torch), 1 without a scale, the weight in affine mode; a = shift / bias.

    Bound, with D the row width, rstd = 1 / sqrt(var + eps):
      * the fp32 mean: a sum of D terms in any order has partial sums of size sqrt(D) rms(x) + D |mean| at most, each add rounds by
        2^-24 of it, independent roundings add to sqrt(D) of them; divided by D (one more rounding, inside C):
        |d mean| <= C sqrt(D) 2^-24 (rms(x) + |mean|)  [rms(x) / sqrt(D) would do for the zero-mean part; the looser form is kept],
        and it moves y by |d mean| rstd |m|;
      * the sum of squares of (x - mean): all terms positive, relative error C sqrt(D) 2^-24, halved by the square root; then the
        division by D and the + eps (half each after the root), rsqrtf (2 ulp = 4 * 2^-24), the rounding of x - mean, of * rstd, of * m:
        (C sqrt(D) / 2 + 8) 2^-24 relative to |z m|  (the error of the mean enters the sum of squares only in second order:
        sum (x - mean) = 0);
      * the final add (or the FMA it contracts to): 2^-24 (|z m| + |a|), its |z m| part counted in the 8 above;
      * one bf16 ulp for the store."""
    x64 = x.double()
    D = x.shape[-1]
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (x64 - mean) * rstd
    if mul is None:
        m = torch.ones(D, dtype=torch.float64, device=x.device)
    elif affine:
        m = mul.double()
    else:
        m = (1.0 + mul.float()).to(BF16).double()
    a = torch.zeros(D, dtype=torch.float64, device=x.device) if add is None else add.double()
    y = z * m + a
    rms = torch.sqrt((x64 ** 2).mean(-1, keepdim=True))
    bound = (ulp_out(y, BF16) + C * math.sqrt(D) * EPS32 * (rms + mean.abs()) * rstd * m.abs()
             + (0.5 * C * math.sqrt(D) + 8.0) * EPS32 * (z * m).abs() + EPS32 * a.abs())
    return y, bound


# ---------------------------------------------------------------------------------------------------- RMSNorm + gain + RoPE
def _rbf(t64):
    return t64.to(BF16).double()


def near_bf16_tie(t64, rel: float = 2.0 ** -20):
    """t64 within rel * |t64| of the midpoint of two neighbouring bf16 values"""
    u = ulp_out(t64, BF16)
    frac = t64.abs() / u
    return ((frac - torch.floor(frac)) - 0.5).abs() * u <= rel * t64.abs()


def qknorm_ref(x, w, cos=None, sin=None, n_rope: int = 0, eps: float = 1e-6):
    """x [rows, heads, 128] bf16, w [heads, 128] bf16 (the q gain for q heads, the k gain for k heads), cos / sin [>= n_rope, 128].
    The contract has two intermediate bf16 roundings, y = bf16(bf16(x r) w), r = rsqrt(mean(x^2) + eps), and then ONE fp32 RoPE
    expression rounded once: o[2i] = y[2i] c[2i] - y[2i+1] s[2i], o[2i+1] = y[2i+1] c[2i+1] + y[2i] s[2i+1] for rows < n_rope.
    The chain is computed in fp64 WITH those roundings.  A legitimate fp32-level difference in r (the sum of 128 squares in any order:
    C sqrt(128) 2^-24 / 2, plus rsqrtf and two multiplies: < 2^-20 relative) can flip an intermediate rounding by a whole bf16 ulp
    when the fp64 intermediate lies within 2^-20 relative of a rounding tie: such an element - for a RoPE row either element of its
    pair - is AMBIGUOUS and left out of the bound (the caller still requires it finite and within 2 ulp).  Everywhere else y is known
    exactly, and
      * a RoPE row computes two exact-operand products, each rounded (2^-24 of it), and their sum, rounded (2^-24 of at most the sum
        of the two magnitudes) - or one rounding less with an FMA: |err| <= ulp_bf16(o64) + 3 * 2^-24 (|y0 c| + |y1 s|);
      * any other row stores y: ulp_bf16 + 2^-24 |y| (in fact exact).
    An ambiguous element may carry a flip of one ulp of its intermediate bf16(x r): through the gain (|w| < 2) that is at most 2 ulp of y,
    and a rotation carries it to o scaled by |c| and |s|: amb_bound = 2 ulp_bf16(y) for a plain row, bound + 2 (ulp(y0) |c| + ulp(y1) |s|)
    for a RoPE row ("within 2 ulp", the ulp taken where the flip happens: o itself can be small by cancellation).
    Returns (o64, bound, ambiguous, amb_bound)."""
    x64 = x.double()
    r = 1.0 / torch.sqrt((x64 ** 2).mean(-1, keepdim=True) + eps)
    t1 = x64 * r
    y1 = _rbf(t1)
    t2 = y1 * w.double()[None]
    y = _rbf(t2)
    amb = near_bf16_tie(t1)         # t2 = y1 * w is a product of two bf16 values: exact in fp32 and fp64 alike, its rounding is decided
    o = y.clone()
    bound = ulp_out(y, BF16) + EPS32 * y.abs()
    amb_bound = 2.0 * ulp_out(y, BF16)
    if n_rope > 0:
        c, s = cos[:n_rope].double()[:, None, :], sin[:n_rope].double()[:, None, :]
        yr = y[:n_rope]
        y0, y1_ = yr[..., 0::2], yr[..., 1::2]
        oe = y0 * c[..., 0::2] - y1_ * s[..., 0::2]
        oo = y1_ * c[..., 1::2] + y0 * s[..., 1::2]
        o[:n_rope] = torch.stack([oe, oo], dim=-1).flatten(-2)
        me = (y0 * c[..., 0::2]).abs() + (y1_ * s[..., 0::2]).abs()
        mo = (y1_ * c[..., 1::2]).abs() + (y0 * s[..., 1::2]).abs()
        mag = torch.stack([me, mo], dim=-1).flatten(-2)
        bound[:n_rope] = ulp_out(o[:n_rope], BF16) + 3.0 * EPS32 * mag
        ue, uo = ulp_out(y0, BF16), ulp_out(y1_, BF16)
        fe = ue * c[..., 0::2].abs() + uo * s[..., 0::2].abs()
        fo = uo * c[..., 1::2].abs() + ue * s[..., 1::2].abs()
        amb_bound[:n_rope] = bound[:n_rope] + 2.0 * torch.stack([fe, fo], dim=-1).flatten(-2)
        ar = amb[:n_rope]
        pair = ar[..., 0::2] | ar[..., 1::2]
        amb = amb.clone()
        amb[:n_rope] = torch.stack([pair, pair], dim=-1).flatten(-2)
    return o, bound, amb, amb_bound


# ---------------------------------------------------------------------------------------------------- timestep embedding
def timestep_ref(t, dim: int, max_period: float = 10000.0):
    """a64 = fp32(t) exp(-ln(P) i / half) in fp64, out = [cos a64 | sin a64].  Bound: ulp_bf16(y64) + |a64| rho + 2^-22.
    rho is the relative error of the kernel's fp32 argument, per frequency i, with e_i = ln(P) i / half the exponent:
      logf: 1 ulp, 2^-23 relative to ln P, i.e. 2^-23 e_i absolute in the exponent;
      the multiply by i: 2^-24 e_i;  the divide by half (1 ulp where not correctly rounded): 2^-23 e_i;
      expf turns an absolute error d of its argument into a relative error d of its value and adds 1 ulp of its own: 2^-23;
      the multiply by t: 2^-24;
      rho_i = (5 e_i + 3) 2^-25, at most (5 * 9.21 + 3) 2^-25 = 6.1 * 2^-22 for P = 10000.
    d cos(a) <= |d a| = |a64| rho; cosf / sinf themselves (2 ulp at values <= 1): 2^-22."""
    t64 = t.reshape(-1).to(F32).double()
    half = dim // 2
    i = torch.arange(half, dtype=torch.float64, device=t.device)
    e = math.log(max_period) * i / half
    a = t64[:, None] * torch.exp(-e)[None]
    y = torch.cat([torch.cos(a), torch.sin(a)], dim=-1)
    rho = (5.0 * e + 3.0) * 2.0 ** -25
    da = (a.abs() * rho[None]).repeat(1, 2)
    return y, ulp_out(y, BF16) + da + 2.0 ** -22


# ---------------------------------------------------------------------------------------------------- small-M linear, masked mean
def silu64(x):
    x64 = x.double()
    return x64 / (1.0 + torch.exp(-x64))


def tie_free_for_silu(x):
    """x (bf16) with the few elements replaced whose silu_64(x) lies within 2^-16 relative of a bf16 rounding tie: the operand
    bf16(silu(x)) of a silu_in linear is then the same for every evaluation of SiLU that is good to 2^-16, i.e. known exactly"""
    x = x.clone()
    x[near_bf16_tie(silu64(x), 2.0 ** -16)] = 0.75
    assert not bool(near_bf16_tie(silu64(x), 2.0 ** -16).any())
    return x


def masked_mean_ref(x, mask=None) -> Ref:
    """out[d] = sum_l x[l][d] mask[l] / sum_l mask[l]: error_bounds.gemm_ref over K = L with the operand a[l] = mask[l] / count (exact
    products x * 0 and x * 1 in the kernel; its one division is a rounding inside C)."""
    L = x.shape[0]
    m = torch.ones(L, dtype=torch.float64, device=x.device) if mask is None else mask.double()
    return gemm_ref((m / m.sum())[None], x.double().T.contiguous())


# ---------------------------------------------------------------------------------------------------- Euler step
def euler_ref(s, v, dt: float):
    """|got - (s + v dt)_64| <= 2^-24 (|y64| + |v dt|): the product rounded (2^-24 |v dt|) and the sum rounded (2^-24 |y|), or the one
    rounding of the FMA hipcc may contract them to - both orders of evaluation are inside.  dt is the fp32 value the kernel receives."""
    dt32 = float(torch.tensor(dt, dtype=F32))
    p = v.double() * dt32
    y = s.double() + p
    return y, EPS32 * (y.abs() + p.abs()) + 2.0 ** -149


# ---------------------------------------------------------------------------------------------------- GroupNorm apply
def silu_e32(t64, y64):
    """the fp32 error of silu_f on an exact argument t (derived in gn_apply_ref): |y| ((|t| + 2) 2^-24 + 2^-22)"""
    return y64.abs() * ((t64.abs() + 2.0) * EPS32 + 2.0 ** -22)


def gn_apply_eval(x, affine, silu: bool):
    """(y64, e32): the fp64 value of gn_apply_ref and the error of its fp32 evaluation alone (the bound without the store's ulp)"""
    sc, sh = affine[:, 0].double()[None], affine[:, 1].double()[None]
    p = x.double() * sc
    t = p + sh
    lin = 2.0 ** -23 * (p.abs() + sh.abs())
    if not silu:
        return t, lin
    y = silu64(t)
    return y, 1.1 * lin + silu_e32(t, y)


def gn_apply_ref(x, affine, silu: bool):
    """t = x sc + sh from the fp32 affine values, y = silu(t) or t, in fp64.
    t in fp32: the product rounded (2^-24 |x sc|) and the sum (2^-24 |t| <= 2^-24 (|x sc| + |sh|)): 2^-23 (|x sc| + |sh|) covers both
    and the FMA.  SiLU's slope is at most 1.1 in magnitude, so that error reaches y times 1.1.  silu_f = t * rcp(1 + __expf(-t)):
    __expf(-t) = exp2(-t log2 e) rounds its argument (|t| 2^-24 relative to the value) and is 1 ulp (2^-23) itself; that relative error
    reaches the sigmoid times (1 - sigmoid) <= 1; the add, v_rcp_f32 (1 ulp) and the multiply: 2^-24 + 2^-23 + 2^-24:
    |y| ((|t| + 2) 2^-24 + 2^-22).  One fp16 ulp for the store."""
    y, e32 = gn_apply_eval(x, affine, silu)
    return y, ulp_out(y, F16) + e32


# ---------------------------------------------------------------------------------------------------- row softmax
def softmax_ref(s, valid, scale: float):
    """p64 = softmax over the first valid[r] columns of scale * s[r] in fp64; zero behind them.
    Bound: ulp_f16(p64), floored at the subnormal spacing 2^-24 (ulp_out's floor for fp16), plus p64 times
      C sqrt(valid) 2^-24   the fp32 sum of `valid` positive terms in any order,
      |scale s - m| 2^-22   __expf(a) = exp2(a log2 e): the argument a = scale s - m is rounded twice on the way (the subtract or FMA
                            and the multiply by log2 e), an absolute error of 2 * 2^-24 |a| in the exponent for the numerator and up to
                            the same in the dominant terms of the denominator: it grows with the distance from the row maximum,
      2^-21                 exp2 (1 ulp) in numerator and denominator, the reciprocal and the final multiply."""
    rows, cols = s.shape
    col = torch.arange(cols, device=s.device)[None]
    ok = col < valid[:, None]
    a = torch.where(ok, s.double() * float(torch.tensor(scale, dtype=F32)), torch.full((), -math.inf, dtype=torch.float64, device=s.device))
    m = a.max(-1, keepdim=True).values
    e = torch.exp(a - m)
    p = e / e.sum(-1, keepdim=True)
    dist = torch.where(ok, (a - m).abs(), torch.zeros_like(a))
    bound = ulp_out(p, F16) + p * (C * torch.sqrt(valid.double())[:, None] * EPS32 + dist * 2.0 ** -22 + 2.0 ** -21)
    return p, bound


# ---------------------------------------------------------------------------------------------------- temporal average
def temporal_avg_ref(x, T_in: int, HW: int, k: int, s: int):
    """x [T_in * HW, C] fp16 -> the fp64 mean of the k frames t s + i - (k - 1), clamped at 0 (replicate pad in front), for t < T_out.
    Bound: ulp_f16 + (k + 1) 2^-24 max|x|: k - 1 fp32 adds of partial sums below k max|x|, each rounding 2^-24 of one, taken relative
    to the mean (divided by k): (k - 1) 2^-24 max|x|; the reciprocal 1 / k and the multiply by it: 2 * 2^-24 max|x|."""
    C_ = x.shape[1]
    x64 = x.double().reshape(T_in, HW, C_)
    t_out = (T_in - 1) // s + 1
    idx = (torch.arange(t_out)[:, None] * s + torch.arange(k)[None] - (k - 1)).clamp(min=0).to(x.device)
    g = x64[idx]                                   # [t_out, k, HW, C]
    y = g.mean(1).reshape(t_out * HW, C_)
    mx = g.abs().amax(1).reshape(t_out * HW, C_)
    return y, ulp_out(y, F16) + (k + 1) * EPS32 * mx


# ---------------------------------------------------------------------------------------------------- data classes and shapes
# (shared by the CPU proof and the GPU tests, so that what is asserted about the data on the CPU holds for the data the GPU sees)
LN_DS = [8, 504, 512, 520, 1000, 2048, 2056, 3072, 3080, 4096]     # both sides of every MAXC boundary, a ragged last chunk group
LN_CLASSES = ["control", "offset", "massive", "constant"]
QK_HEADS = [1, 8, 9, 24]                                          # 2H = 16: one trip of the head loop; 18: one trip and a ragged one
QK_ROWS = [(5, 0), (5, 1), (5, 4), (5, 5)]                        # (n_rows, n_rope)
QK_CLASSES = ["control", "massive"]


def data_rows(cls: str, M: int, D: int, key: str) -> torch.Tensor:
    """bf16 rows [M, D] (CPU) of one data class: control (hashed uniform, unit variance), offset (500 +- 1), massive (the DiT pattern
    of test_gpu_groupnorm_conditioning.dit_rows: a few channels at +-1000..3000, offset rows, a constant row), constant, tiny (2^-20)"""
    from hunyuanvideo_efficiency_amd import synthetic as syn
    u = syn.hashed_uniform((M, D), f"{key}.{cls}", 23) * math.sqrt(3.0)
    if cls == "control":
        x = u
    elif cls == "offset":
        x = 500.0 + u
    elif cls == "massive":
        from tests.test_gpu_groupnorm_conditioning import dit_rows
        if D >= 32:
            return dit_rows(max(M, 5), D, f"{key}.{cls}")[:M].contiguous()
        x = syn.hashed_uniform((max(M, 5), D), f"{key}.{cls}", 23) * math.sqrt(3.0)     # dit_rows needs 18 columns: its pattern, folded
        u5 = x.clone()
        x[0, [3, D // 2]] = torch.tensor([2800.0, -1500.0])
        x[1, 17 % D] = -3000.0
        x[2], x[3], x[4] = 500.0 + u5[2], 0.3, -500.0 + u5[4]
        x = x[:M]
    elif cls == "constant":
        x = torch.tensor([0.3, -1.75, 500.0, 2.0 ** -10, -96.0, 7.0, 0.0, 1.0, -0.011])[:M, None].expand(M, D)
    elif cls == "tiny":
        x = u * 2.0 ** -20
    else:
        raise KeyError(cls)
    return x.to(BF16).contiguous()


def rope_tables_independent(rows: int, key: str):
    """cos / sin [rows, 128] fp32 with an independent value in every column: a kernel that reads one column for both elements of a
    pair (as the real tables, cos[2i] == cos[2i+1], would allow) fails on them"""
    from hunyuanvideo_efficiency_amd import synthetic as syn
    return (syn.hashed_uniform((rows, 128), key + ".cos", 29).contiguous(), syn.hashed_uniform((rows, 128), key + ".sin", 31).contiguous())


# ---------------------------------------------------------------------------------------------------- operands shared by the CPU proof
# and the GPU tests
def _syn():
    from hunyuanvideo_efficiency_amd import synthetic as syn
    return syn


def _u(shape, key, scale=1.0):
    return _syn().hashed_uniform(shape, key, 41) * (scale * math.sqrt(3.0))


def qk_case(cls, H, n_rows, key):
    ld = 3 * H * 128 + 64
    k_off = H * 128 + 128
    row = data_rows(cls, n_rows, ld, key)
    x = torch.cat([row[:, :H * 128], row[:, k_off:k_off + H * 128]], 1).reshape(n_rows, 2 * H, 128).contiguous()
    qw, kw = (1.0 + _u((128,), key + ".qw", 0.2)).to(BF16), (1.0 + _u((128,), key + ".kw", 0.2)).to(BF16)
    w = torch.cat([qw.expand(H, 128), kw.expand(H, 128)], 0)
    return row, x, w, qw, kw


def gemv_operands(M, N, K, key):
    return _u((M, K), key + ".x").to(BF16), _u((N, K), key + ".w", 0.5 / math.sqrt(K)).to(BF16), _u((N,), key + ".b", 0.05).to(BF16)


TS = [0.0, 1e-3, 0.5, 1.0, 499.5, 999.0, 1000.0]


def softmax_scores(cls, rows, cols, key):
    u = _syn().hashed_uniform((rows, cols), f"{key}.{cls}", 43)
    if cls == "flat":
        return (u * 0.25).contiguous()
    if cls == "peaked":
        s = u.clone()
        s[torch.arange(rows), (torch.arange(rows) * 7) % cols] += 40.0       # one score 40 above the rest, inside the first frame or not
        return s.contiguous()
    if cls == "spread":
        return (u * 60.0).contiguous()
    raise KeyError(cls)


SOFTMAX_CLASSES = ["flat", "peaked", "spread"]


def valid_of(rows, cols, causal_block):
    r = torch.arange(rows)
    return torch.full((rows,), cols) if causal_block == 0 else torch.clamp((r // causal_block + 1) * causal_block, max=cols)
