"""fp64 reference and per-element error bound of the linear temporal interpolation (csrc/hv_temporal.hip, include/hv_temporal.h), in the
conventions of tests/rowwise_bounds.py, whose helpers it uses (ulp_out, EPS32 = 2^-24, check, mismatch_share).
tests/test_tinterp_bounds_cpu.py shows what the bound accepts and what it rejects; tests/test_gpu_tinterp.py holds the kernel to it.

The rule (F.interpolate(scale_factor=(s,1,1), mode="trilinear", align_corners=False) on a 5-D input, integer s).  Output frame t:
    num = max(2 t + 1 - s, 0),  t0 = num // (2 s),  t1 = min(t0 + 1, T_in - 1),  lambda = (num mod 2 s) / (2 s),
    y = (1 - lambda) x[t0] + lambda x[t1].
The reference is this rule in fp64 on the exact fp16 inputs with the exact rational lambda (a quotient of two small integers: the fp64
division is its nearest double, 2^-53 relative, nothing against the terms below).

The bound:  |got - y64| <= ulp16(y64) + E32 (|x0| + |x1|) + DLAMBDA(t) |x1 - x0|.

  E32 = 3 * 2^-24.  The fp32 evaluation of the blend, every rounding 2^-24 of the magnitude it rounds (EPS32), in each association:
    x0 + lambda (x1 - x0)        d = x1 - x0 rounds by 2^-24 |d| (times lambda < 1), the product by 2^-24 |lambda d| <= 2^-24 |d|, the sum
                                 by 2^-24 |y|:  2^-24 (2 |x1 - x0| + |y|) <= 2^-24 * 3 (|x0| + |x1|)          (|y| <= max(|x0|, |x1|));
    (1 - lambda) x0 + lambda x1  w0 = 1 - lambda rounds by 2^-25 (w0 <= 1): 2^-25 |x0|; the two products by 2^-24 (|w0 x0| + |lambda x1|)
                                 <= 2^-24 (|x0| + |x1|); the sum by 2^-24 |y|:  <= 2^-24 * 2.5 (|x0| + |x1|);
    the same with an FMA         one rounding fewer.
  DLAMBDA(t) = 4 * 2^-23 (src + 1/2), src = num / (2 s) the source coordinate: the error of the weight itself, which moves y by
  |x1 - x0| times it.  The kernel forms lambda from the integers with one correctly rounded division: 2^-25 at most.  torch forms it in
  fp32 as src32 - floor(src32), src32 = (1 / s)_32 * (t + 1/2) - 1/2: the reciprocal is off by 2^-24 relative, the product (of size
  src + 1/2) rounds by another 2^-24 of itself, the subtraction of 1/2 and of the floor are exact - 2^-23 (src + 1/2) absolute, which
  grows with the frame index where the kernel's does not.  Measured on CPU torch over T = 1..19, s = 1..6: 0.62 of that (1.3e-6 at
  T = 18, s = 3).  The factor 4 is the margin for a build of torch that spends more roundings on the coordinate (a reciprocal taken
  in two steps, a fused multiply-subtract of the 1/2 and a separate one): DLAMBDA stays below 1e-5 for T <= 19, forty times below the
  2^-12 by which a weight rounded to fp16 is off, and far below every indexing mistake (1 / (2 s) at least).

Copies.  Where lambda == 0 or t0 == t1 the output must have the bits of x[t0] (`copies`): s == 1, the clamped leading frames
(t < s / 2) and the clamped trailing ones.  The bound there is ulp16 only by construction (x1 == x0 or DLAMBDA multiplies nothing the
rule uses), but the GPU test asserts equality of bits.

Exactness of the one rounding (mismatch_share).  A one-ulp bound cannot tell one rounding to fp16 from two (products rounded to fp16
first move a result by half an ulp).  The share of outputs whose bits differ from round-to-nearest-even of y64 can: a faithful fp32
evaluation differs only where its fp32 error carries a value across an fp16 rounding tie, about E32-level / 2^-11 = 2^-11 of the
outputs.  Measured on the CPU (test_mismatch_share_of_faithful_emulations: the data and every shape class of the GPU test, the three
association orders): largest 0.0049 at T_in = 9, s = 3, FMA form (MEASURED_SHARE = 0.005); the cap is 4 x that, never below 2 / numel - the factor 4 covers an order or a
data draw unluckier than the sampled ones.  The mutant that rounds the products to fp16 reaches 0.2."""
from __future__ import annotations

import math

import torch

from tests.rowwise_bounds import EPS32, F16, check, mismatch_share, ratio, ulp_out  # noqa: F401

E32 = 3.0 * EPS32
MEASURED_SHARE = 0.005          # largest share of a faithful fp32 emulation (tests/test_tinterp_bounds_cpu.py measures it)


def mismatch_cap(numel: int) -> float:
    return max(4.0 * MEASURED_SHARE, 2.0 / numel)


def dlambda(src: torch.Tensor) -> torch.Tensor:
    return 4.0 * 2.0 ** -23 * (src + 0.5)


def frames(T_in: int, s: int):
    """per output frame t < T_in * s: (t0, t1, numerator of lambda) as int64 tensors; lambda = numerator / (2 s)"""
    t = torch.arange(T_in * s, dtype=torch.int64)
    num = (2 * t + 1 - s).clamp(min=0)
    t0 = num // (2 * s)
    return t0, (t0 + 1).clamp(max=T_in - 1), num % (2 * s)


def copies(T_in: int, s: int) -> torch.Tensor:
    """bool [T_in * s]: the output frames that are bit copies of x[t0]"""
    t0, t1, r = frames(T_in, s)
    return (r == 0) | (t0 == t1)


def tinterp_ref(x: torch.Tensor, T_in: int, HW: int, s: int):
    """x [T_in * HW, C] fp16 -> (y64 [T_in * s * HW, C], bound) of the rule above"""
    C_ = x.shape[1]
    x64 = x.double().reshape(T_in, HW, C_)
    t0, t1, r = (v.to(x.device) for v in frames(T_in, s))
    lam = (r.double() / (2 * s))[:, None, None]
    src = (t0.double() + r.double() / (2 * s))[:, None, None]
    x0, x1 = x64[t0], x64[t1]
    y = (1.0 - lam) * x0 + lam * x1
    bound = ulp_out(y, F16) + E32 * (x0.abs() + x1.abs()) + dlambda(src) * (x1 - x0).abs()
    return y.reshape(T_in * s * HW, C_), bound.reshape(T_in * s * HW, C_)


def activations(T_in: int, HW: int, C_: int, key: str) -> torch.Tensor:
    """fp16 rows [T_in * HW, C] (CPU): hashed uniform values of unit variance, the scale of a GroupNorm'd activation"""
    from hunyuanvideo_efficiency_amd import synthetic as syn
    return (syn.hashed_uniform((T_in * HW, C_), f"tinterp.{key}.{T_in}.{HW}.{C_}", 47) * math.sqrt(3.0)).to(F16)


# the shapes of tests/test_gpu_tinterp.py (the issue's grid); the CPU test measures the emulations on the same
T_INS, SCALES, HWS, CS = (1, 2, 3, 5, 9), (1, 2, 3, 4), (1, 7, 12), (8, 64, 72, 128)
