"""CPU: what the bound of tests/tinterp_bounds.py accepts (faithful fp32 evaluations of the rule in three association orders, CPU torch's
own trilinear F.interpolate) and what it rejects (the ways such a kernel can be subtly wrong), and the share of outputs whose bits differ
from the correctly rounded fp64 value."""
import pytest
import torch
import torch.nn.functional as F

from tests import tinterp_bounds as B

F16, F32 = torch.float16, torch.float32
ORDERS = ("lerp", "weights", "fma")
MUTANTS = ("align_corners", "nearest", "swapped", "no_half_pixel", "no_front_clamp", "no_end_clamp", "lambda_f16", "products_f16")


def evaluate(x, T_in, HW, s, order="weights", mutant=None):
    """the rule in fp32 on x [T_in * HW, C] fp16 -> fp16 [T_in * s * HW, C]; `mutant` breaks it in one way"""
    C_ = x.shape[1]
    xf = x.float().reshape(T_in, HW, C_)
    t = torch.arange(T_in * s, dtype=torch.int64)
    if mutant == "align_corners":          # src = t (T_in - 1) / (T_out - 1)
        den = max(T_in * s - 1, 1)
        num = t * (T_in - 1)
    elif mutant == "no_half_pixel":        # src = t / s
        den, num = s, t
    elif mutant == "no_front_clamp":       # src may be negative: t0 = -1 is read as frame 0 with a negative weight on it (extrapolation)
        den, num = 2 * s, 2 * t + 1 - s
    else:
        den, num = 2 * s, (2 * t + 1 - s).clamp(min=0)
    t0 = torch.div(num, den, rounding_mode="floor")
    r = num - t0 * den
    if mutant == "no_front_clamp":
        t0, r = torch.where(num < 0, torch.zeros_like(t0), t0), torch.where(num < 0, num, r)
    t1 = t0 + 1
    if mutant == "no_end_clamp":           # reads the frame behind the last one: here it wraps to frame 0
        t1 = t1 % T_in
    else:
        t1 = t1.clamp(max=T_in - 1)
    t0 = t0.clamp(max=T_in - 1)
    lam = (r.to(F32) / torch.tensor(float(den), dtype=F32))[:, None, None]
    if mutant == "lambda_f16":
        lam = lam.to(F16).float()
    if mutant == "nearest":
        return xf[torch.div(t, s, rounding_mode="floor")].to(F16).reshape(-1, C_)
    x0, x1 = (xf[t1], xf[t0]) if mutant == "swapped" else (xf[t0], xf[t1])
    if mutant == "products_f16":
        y = ((1.0 - lam) * x0).to(F16).float() + (lam * x1).to(F16).float()
    elif order == "lerp":
        y = x0 + lam * (x1 - x0)
    elif order == "weights":
        y = (1.0 - lam) * x0 + lam * x1
    else:                                  # fmaf(lam, x1, w0 * x0): the product lam * x1 is exact in fp64 (24 x 11 bits)
        y = (lam.double() * x1.double() + ((1.0 - lam) * x0).double()).float()
    return y.to(F16).reshape(-1, C_)


def cases():
    return [(T, s) for T in range(1, 20) for s in range(1, 7)]


def test_reference_is_the_rule_spelled_out():
    x = B.activations(3, 2, 8, "spell")
    y, _ = B.tinterp_ref(x, 3, 2, 2)
    x64 = x.double().reshape(3, 2, 8)
    want = torch.stack([x64[0], 0.75 * x64[0] + 0.25 * x64[1], 0.25 * x64[0] + 0.75 * x64[1], 0.75 * x64[1] + 0.25 * x64[2],
                        0.25 * x64[1] + 0.75 * x64[2], x64[2]]).reshape(12, 8)
    assert torch.equal(y, want)
    assert B.copies(3, 2).tolist() == [True, False, False, False, False, True]
    assert B.copies(4, 1).all() and B.copies(1, 5).all()
    assert B.copies(3, 3).tolist() == [True, True, False, False, True, False, False, True, True]      # lambda == 0 at t = 1, 4, 7


@pytest.mark.parametrize("order", ORDERS)
def test_bound_accepts_faithful_fp32_evaluations(order):
    worst = 0.0
    for T, s in cases():
        x = B.activations(T, 3, 8, "accept")
        y64, bound = B.tinterp_ref(x, T, 3, s)
        got = evaluate(x, T, 3, s, order)
        worst = max(worst, B.check(got, y64, bound, f"{order} T={T} s={s}"))
        cp = B.copies(T, s).repeat_interleave(3)
        assert torch.equal(got[cp].view(torch.int16), y64.to(F16)[cp].view(torch.int16))
    assert worst <= 1.0


def test_bound_accepts_torch_trilinear():
    worst, worst_lam = 0.0, 0.0
    for T, s in cases():
        x = B.activations(T, 3, 8, "torch")
        y64, bound = B.tinterp_ref(x, T, 3, s)
        x5 = x.float().reshape(T, 3, 8).permute(2, 0, 1)[None, :, :, :, None]                    # [1, C, T, HW, 1]
        got = F.interpolate(x5, scale_factor=(s, 1, 1), mode="trilinear", align_corners=False)[0, :, :, :, 0].permute(1, 2, 0)
        worst = max(worst, B.check(got.reshape(-1, 8).to(F16), y64, bound, f"torch T={T} s={s}"))
        # and the weight alone, against the room DLAMBDA gives it (one-hot frames make the output the weight)
        eye = torch.eye(T)[None, None, :, :, None]
        w = F.interpolate(eye, scale_factor=(s, 1, 1), mode="trilinear", align_corners=False)[0, 0, :, :, 0].double()
        t0, t1, r = B.frames(T, s)
        live = t0 != t1
        lam = r.double() / (2 * s)
        err = (w[torch.arange(T * s), t1] - lam).abs()[live]
        if err.numel():
            worst_lam = max(worst_lam, float((err / B.dlambda(t0.double() + lam)[live]).max()))
    assert worst <= 1.0 and worst_lam <= 0.5, (worst, worst_lam)


def test_nearest_exact_and_area_are_nearest():
    """what AutoencoderKLCausal3D._interp_op relies on"""
    for T, s in cases():
        x5 = B.activations(T, 3, 8, "modes").float().reshape(T, 3, 8).permute(2, 0, 1)[None, :, :, :, None]
        n = F.interpolate(x5, scale_factor=(s, 1, 1), mode="nearest")
        for mode in ("nearest-exact", "area"):
            assert torch.equal(F.interpolate(x5, scale_factor=(s, 1, 1), mode=mode), n), (mode, T, s)
    for mode in ("linear", "bilinear", "bicubic"):
        with pytest.raises((NotImplementedError, ValueError, RuntimeError)):
            F.interpolate(torch.zeros(1, 1, 2, 1, 1), scale_factor=(2, 1, 1), mode=mode)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_bound_rejects(mutant):
    rejected = 0
    for T, s in [(5, 2), (5, 3), (9, 3), (9, 4), (19, 5), (7, 6)]:
        x = B.activations(T, 7, 64, "reject")
        y64, bound = B.tinterp_ref(x, T, 7, s)
        got = evaluate(x, T, 7, s, mutant=mutant)
        bad = float((B.ratio(got, y64, bound) > 1.0).double().mean())
        if mutant == "products_f16":
            # half-ulp damage: outside the bound on a few elements, plainly visible in the share of mismatching bits
            share = B.mismatch_share(got, y64, F16)
            assert share > 0.1 > B.mismatch_cap(got.numel()), (T, s, share)
        rejected += bad > 0
        if mutant not in ("products_f16", "lambda_f16"):
            assert bad > 0.01, (mutant, T, s, bad)
    # a weight rounded to fp16 is exact for s = 2 (1/4, 3/4) and s = 4 (eighths): it must fall on the others
    assert rejected >= (3 if mutant == "lambda_f16" else 6), (mutant, rejected)


def test_mismatch_share_of_faithful_emulations():
    """the figure behind MEASURED_SHARE: every shape class of the GPU test, the three orders"""
    worst = (0.0, ())
    for T in B.T_INS:
        for s in B.SCALES:
            x = B.activations(T, 12, 128, "share")
            y64, _ = B.tinterp_ref(x, T, 12, s)
            for order in ORDERS:
                share = B.mismatch_share(evaluate(x, T, 12, s, order), y64, F16)
                worst = max(worst, (share, (T, s, order)))
                assert share <= B.mismatch_cap(y64.numel()), (T, s, order, share)
    print("largest share", worst)
    assert worst[0] <= B.MEASURED_SHARE, worst
    assert worst[0] >= B.MEASURED_SHARE / 4 or B.MEASURED_SHARE == 0.0, f"MEASURED_SHARE is stale: {worst}"
