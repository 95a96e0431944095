"""fp64 reference of a GEMM-shaped reduction y[m, n] = sum_k a[m, k] w[n, k] (+ b[n]) and a per-element error bound for a kernel
that multiplies exactly (bf16, fp16 and e4m3 products are exact in fp32) and accumulates in fp32, in ANY order, then stores once.

    |got - y64| <= ulp_out(y64) + C * sqrt(K) * 2^-24 * P

  * ulp_out: spacing of the output format at |y64|, floored at its smallest normal (bf16 2^-133, fp16 2^-24); for fp32 outputs
    2^-23 |y64|.  Covers the one final rounding (half an ulp) plus an accumulation error that straddles a binade edge.
  * P = ||(a_k w_k)_k||_2 + |y64| + |b|: the size of a partial sum of the K products taken in a random order (a random walk of
    the zero-mean part, plus a drift towards y).  The first-order fp32 summation error is sum_j eps_j s_j with |eps_j| <= 2^-24
    and s_j the partial sums; for independent eps_j its spread is <= 2^-24 sqrt(K) max|s_j|.  |b| also covers the one rounding of
    acc * scale (fp8 row and tensor scales) and of acc + bias.
  * C = 4 everywhere.  THIS IS A STATISTICAL BOUND FOR RANDOM DATA, NOT A WORST-CASE ONE: an adversarial order of adversarial
    data (all positive products first) has partial sums up to S = sum_k |a_k w_k| and could exceed it.  The worst-case form
    (P = S) is sqrt(K) looser: with it, a correct fp32-output kernel used < 1 % of the bound, which leaves no room to see anything.
  * worst_case=True selects P = S + |b|.  For the fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4), whose 128-term reduction is not
    as exact as fp32 adds: on random data its near-zero outputs miss the statistical bound by up to 3.5x (errors ~2^-19 S,
    scattered over every row and column range, i.e. not a tile effect); the worst-case form holds them with a ratio of ~0.3.

What it rejects (tests/test_error_bounds_cpu.py): rounding the running sum to the 16-bit output format once per 64-wide K-tile
(each rounding adds up to half an ulp of the partial sum: sqrt(K/64) of them exceed the one ulp allowed), a dropped K-tile, and
a 16-row fragment read one row off.  What it accepts: fp32 accumulation in any order."""
from __future__ import annotations

import math
from typing import Optional

import torch

C = 4.0
EPS32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)

# (mantissa bits, smallest normal exponent) of each output format
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def ulp_out(y64: torch.Tensor, dtype) -> torch.Tensor:
    """spacing of `dtype` at |y64| (fp64), floored at the spacing of its smallest normal; fp32: 2^-23 |y64|"""
    if dtype == torch.float32:
        return y64.abs() * 2.0 ** -23
    mant, emin = _FMT[dtype]
    e = torch.floor(torch.log2(y64.abs().clamp(min=2.0 ** emin)))
    return torch.exp2(e - mant)


class Ref:
    """fp64 y = sum_k a_k w_k + b, accumulated from K-slices (conv taps, sub-pixel taps), with what the bound needs."""

    def __init__(self):
        self.y = None
        self.sq = None          # sum_k (a_k w_k)^2
        self.s = None           # sum_k |a_k w_k|
        self.k = 0
        self.b = None

    def add(self, a: torch.Tensor, w: torch.Tensor) -> "Ref":
        """a [M, k'] and w [N, k']: the EXACT operand values the kernel multiplied (dequantised where scaled)"""
        a64, w64 = a.double(), w.double()
        y, sq, s = a64 @ w64.T, (a64 * a64) @ (w64 * w64).T, a64.abs() @ w64.abs().T
        self.y = y if self.y is None else self.y + y
        self.sq = sq if self.sq is None else self.sq + sq
        self.s = s if self.s is None else self.s + s
        self.k += a.shape[1]
        return self

    def bias(self, b: Optional[torch.Tensor]) -> "Ref":
        if b is not None:
            b64 = b.double().reshape(1, -1)
            self.y = self.y + b64
            self.b = b64.abs()
        return self

    def bound(self, dtype, worst_case: bool = False) -> torch.Tensor:
        p = self.s.clone() if worst_case else self.sq.sqrt() + self.y.abs()
        if self.b is not None:
            p = p + self.b
        return ulp_out(self.y, dtype) + C * math.sqrt(self.k) * EPS32 * p


def gemm_ref(a, w, b=None) -> Ref:
    return Ref().add(a, w).bias(b)


def ratio(got: torch.Tensor, ref: Ref, dtype, worst_case: bool = False) -> torch.Tensor:
    """|got - y64| / bound per element (inf where got is not finite)"""
    g = got.double().to(ref.y.device)
    r = (g - ref.y).abs() / ref.bound(dtype, worst_case)
    return torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))


def check(got: torch.Tensor, ref: Ref, dtype, what: str = "", worst_case: bool = False) -> float:
    """asserts every element is within the bound; returns the largest error-to-bound ratio"""
    r = ratio(got, ref, dtype, worst_case)
    worst = float(r.max())
    if not worst <= 1.0:
        bad = (r > 1.0).nonzero()
        i = int(r.reshape(-1).argmax())
        m, n = divmod(i, r.shape[1])
        rows, cols = bad[:, 0], bad[:, 1]
        raise AssertionError(f"{what}: {bad.shape[0]} of {r.numel()} elements outside the fp64 error bound (worst ratio {worst:.3g} at "
                             f"[{m}, {n}]: got {float(got.reshape(-1)[i])}, y64 {float(ref.y.reshape(-1)[i]):.9g}); rows "
                             f"[{int(rows.min())}, {int(rows.max())}], cols [{int(cols.min())}, {int(cols.max())}]")
    return worst
