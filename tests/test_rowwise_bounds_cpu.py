"""CPU: the bounds of tests/rowwise_bounds.py have teeth.  For every bounded operation a faithful emulation in torch fp32 - sums taken
in three lane / chunk orders - is accepted on every data class, and the ways such a kernel can be subtly wrong are rejected (at least
one element outside the bound, or a mismatch share above the cap).  The file also asserts the 1 % ambiguity condition of the RMSNorm +
RoPE reference on every data class and shape the GPU test uses, and measures the mismatch share of the faithful emulations that
rowwise_bounds.MEASURED_SHARE records."""
import math

import pytest
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from tests import error_bounds as EB
from tests import rowwise_bounds as RB

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ORDERS = [0, 1, 2]


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 41) * (scale * math.sqrt(3.0))


def rbf(t):
    return t.to(BF16).float()


def sum32(v, order, lanes=64):
    """fp32 sum over the last axis the way a wave takes it: `lanes` running sums (lane l adds elements l, l + lanes, ..), then an xor
    tree.  order 0: the elements as they lie; 1, 2: shuffled (another assignment to lanes and another order within a lane)."""
    n = v.shape[-1]
    if order:
        v = v[..., torch.randperm(n, generator=torch.Generator().manual_seed(order))]
    if order == 2:
        lanes = 16
    pad = (-n) % lanes
    if pad:
        v = torch.cat([v, torch.zeros(*v.shape[:-1], pad, dtype=F32)], -1)      # + 0 is exact
    v = v.reshape(*v.shape[:-1], -1, lanes)
    acc = torch.zeros(*v.shape[:-2], lanes, dtype=F32)
    for i in range(v.shape[-2]):
        acc = acc + v[..., i, :]
    o = lanes // 2
    idx = torch.arange(lanes)
    while o:
        acc = acc + acc[..., idx ^ o]
        o //= 2
    return acc[..., :1]


def outside(got, y64, bound, skip=None):
    r = RB.ratio(got, y64, bound)
    if skip is not None:
        r = r[~skip]
    return int((r > 1.0).sum())


# ---------------------------------------------------------------------------------------------------- LayerNorm + modulate
def ln_emul(x, add, mul, eps=1e-6, order=0, mutant=None, affine=False):
    xf = x.float()
    D = x.shape[-1]
    stat = xf[:, :D - 8] if mutant == "drop_chunk" else xf
    div = float(512 * next(c for c, lim in ((1, 512), (4, 2048), (6, 3072), (8, 4096)) if D <= lim)) if mutant == "padded_width" else float(D)
    mean = sum32(stat, order) / div
    if mutant == "one_pass":
        var = sum32(stat * stat, order) / div - mean * mean
    else:
        d = stat - mean
        var = sum32(d * d, order) / div
    rstd = torch.rsqrt(var + (0.0 if mutant == "no_eps" else eps))
    if mul is None:
        m = torch.ones(D)
    elif affine:
        m = mul.float()
    else:
        m = 1.0 + mul.float() if mutant == "m_unrounded" else rbf(1.0 + mul.float())
    a = torch.zeros(D) if add is None else add.float()
    return ((xf - mean) * rstd * m + a).to(BF16)


def _ln_mod(D, key):
    return U((D,), key + ".shift", 0.5).to(BF16), U((D,), key + ".scale", 0.5).to(BF16)


@pytest.mark.parametrize("cls", RB.LN_CLASSES + ["tiny"])
def test_ln_faithful_accepted(cls):
    for D in RB.LN_DS:
        x = RB.data_rows(cls, 5, D, f"ln.{D}")
        shift, scale = _ln_mod(D, f"ln.{D}")
        y, b = RB.ln_ref(x, shift, scale)
        for o in ORDERS:
            assert outside(ln_emul(x, shift, scale, order=o), y, b) == 0, (cls, D, o)


def test_ln_mutants_rejected():
    # one-pass variance on an offset-500 row.  bf16 holds 500 +- 1 as 498, 500, 502: the squares are multiples of 4 below 2^18 and a
    # power-of-two many of them sum almost exactly in fp32, so the mutant is only weakly wrong at D = 2048 or 4096 (0.5 of the bound);
    # at D = 1000 - a shape of the GPU test - the division leaves E[x^2] = 250001.7 rounded to 2^-6 against a variance of 1.7
    xo = RB.data_rows("offset", 5, 1000, "lnm")
    sh1, sc1 = _ln_mod(1000, "lnm")
    y, b = RB.ln_ref(xo, sh1, sc1)
    for o in ORDERS:
        assert outside(ln_emul(xo, sh1, sc1, order=o), y, b) == 0
        assert outside(ln_emul(xo, sh1, sc1, order=o, mutant="one_pass"), y, b) > 0
    D = 3072
    shift, scale = _ln_mod(D, "lnm")
    for D2 in (520, 1000, 3080):                              # a padded width exists only where D is not the instantiation's limit
        x = RB.data_rows("control", 5, D2, "lnm")
        sh2, sc2 = _ln_mod(D2, "lnm2")
        y2, b2 = RB.ln_ref(x, sh2, sc2)
        assert outside(ln_emul(x, sh2, sc2, mutant="padded_width"), y2, b2) > 0, D2
    x = RB.data_rows("control", 5, 1000, "lnm")
    sh2, sc2 = _ln_mod(1000, "lnm3")
    y2, b2 = RB.ln_ref(x, sh2, sc2)
    assert outside(ln_emul(x, sh2, sc2, mutant="drop_chunk"), y2, b2) > 0
    xc = RB.data_rows("constant", 5, D, "lnm")
    yc, bc = RB.ln_ref(xc, shift, scale)
    assert outside(ln_emul(xc, shift, scale), yc, bc) == 0
    assert torch.equal(yc.to(BF16), shift.expand(5, D)), "a constant row normalises to the shift"
    assert outside(ln_emul(xc, shift, scale, mutant="no_eps"), yc, bc) > 0
    x = RB.data_rows("control", 5, D, "lnm")
    y, b = RB.ln_ref(x, shift, scale)
    share = RB.mismatch_share(ln_emul(x, shift, scale, mutant="m_unrounded"), y, BF16)
    assert share > RB.mismatch_cap("ln.control", x.numel()), share


# ---------------------------------------------------------------------------------------------------- RMSNorm + gain + RoPE
def qk_emul(x, w, cos, sin, n_rope, eps=1e-6, order=0, mutant=None):
    """x [rows, 2H, 128] bf16, w [2H, 128] (q gains then k gains)"""
    xf = x.float()
    H = x.shape[1] // 2
    ss = sum32(xf * xf, order, lanes=16)
    r = torch.rsqrt(ss * (1.0 / 128.0) + eps)
    wf = w.float()[None]
    if mutant == "k_with_q_gain":
        wf = torch.cat([wf[:, :H], wf[:, :H]], 1)
    y = rbf(xf * r * wf) if mutant == "gain_before_cast" else rbf(rbf(xf * r) * wf)
    n = n_rope + 1 if mutant == "rotate_row_n_rope" else n_rope
    if n > 0:
        c, s = cos[:n].float()[:, None], sin[:n].float()[:, None]
        y0, y1 = y[:n, :, 0::2], y[:n, :, 1::2]
        c0, c1, s0, s1 = c[..., 0::2], c[..., 1::2], s[..., 0::2], s[..., 1::2]
        if mutant == "one_cos_column":
            c1 = c0
        oe = y0 * c0 - y1 * s0
        oo = y1 * c1 - y0 * s1 if mutant == "sin_sign" else y1 * c1 + y0 * s1
        if mutant == "rope_rounded_twice":
            oe, oo = rbf(y0 * c0) - y1 * s0, rbf(y1 * c1) + y0 * s1
        y = y.clone()
        y[:n] = torch.stack([oe, oo], -1).flatten(-2)
    return y.to(BF16)


@pytest.mark.parametrize("cls", RB.QK_CLASSES)
def test_qknorm_faithful_accepted_and_ambiguity_below_one_percent(cls):
    for H in RB.QK_HEADS:
        for n_rows, n_rope in RB.QK_ROWS:
            key = f"qk.{H}.{n_rope}"
            _, x, w, _, _ = RB.qk_case(cls, H, n_rows, key)
            cos, sin = RB.rope_tables_independent(n_rows, key)
            y, b, amb, ab = RB.qknorm_ref(x, w, cos, sin, n_rope)
            assert float(amb.float().mean()) <= 0.01, (cls, H, n_rope, float(amb.float().mean()))
            for o in ORDERS:
                got = qk_emul(x, w, cos, sin, n_rope, order=o)
                assert outside(got, y, b, amb) == 0, (cls, H, n_rope, o)
                assert bool(torch.isfinite(got.float()).all())
                assert bool(((got.double() - y).abs() <= ab)[amb].all()), (cls, H, n_rope, o)


def test_qknorm_mutants_rejected():
    H, n_rows, n_rope = 9, 5, 4
    _, x, w, _, _ = RB.qk_case("control", H, n_rows, "qkm")
    cos, sin = RB.rope_tables_independent(n_rows, "qkm")
    y, b, amb, ab = RB.qknorm_ref(x, w, cos, sin, n_rope)
    cap = RB.mismatch_cap("qknorm", x.numel())
    assert outside(qk_emul(x, w, cos, sin, n_rope), y, b, amb) == 0
    for mutant in ("one_cos_column", "sin_sign", "k_with_q_gain", "rotate_row_n_rope"):
        assert outside(qk_emul(x, w, cos, sin, n_rope, mutant=mutant), y, b, amb) > 0, mutant
    for mutant in ("gain_before_cast", "rope_rounded_twice"):
        share = RB.mismatch_share(qk_emul(x, w, cos, sin, n_rope, mutant=mutant), y, BF16, amb)
        assert share > cap, (mutant, share, cap)


# ---------------------------------------------------------------------------------------------------- small-M linear
def silu32(x):
    return x / (1.0 + torch.exp(-x))


def gemv_emul(x, w, b, order=0, silu_in=False, mutant=None):
    a = x.float()
    if silu_in:
        a = silu32(a) if mutant == "silu_in_unrounded" else rbf(silu32(a))
    K = x.shape[1]
    if mutant == "drop_last_chunk":
        a, w, K = a[:, :K - 8], w[:, :K - 8], K - 8
    prod = a[:, None, :] * w.float()[None]                           # [M, N, K]: exact in fp32 for bf16 operands
    if mutant == "bf16_accumulator":                                # the lane accumulators rounded to bf16 after each 512-wide step
        acc = torch.zeros(*prod.shape[:2], 64, dtype=F32)
        for k0 in range(0, K, 512):
            step = prod[..., k0:k0 + 512].reshape(*prod.shape[:2], 64, 8)
            for j in range(8):
                acc = acc + step[..., j]
            acc = rbf(acc)
        r = sum32(acc, 0)[..., 0]
    else:
        r = sum32(prod, order)[..., 0]
    if b is not None:
        r = r + b.float()[None]
    return r.to(BF16)


def test_gemv_faithful_accepted_and_mutants_rejected():
    for K in (8, 256, 512, 520, 3072, 3080):
        x, w, b = RB.gemv_operands(4, 41, K, f"gemv.{K}")
        ref = EB.gemm_ref(x, w, b)
        for o in ORDERS:
            assert float(EB.ratio(gemv_emul(x, w, b, o), ref, BF16).max()) <= 1.0, (K, o)
    x, w, b = RB.gemv_operands(4, 64, 520, "gemvm")
    assert float(EB.ratio(gemv_emul(x, w, b, mutant="drop_last_chunk"), EB.gemm_ref(x, w, b), BF16).max()) > 1.0
    x, w, b = RB.gemv_operands(4, 64, 3072, "gemvm")
    assert float(EB.ratio(gemv_emul(x, w, b, mutant="bf16_accumulator"), EB.gemm_ref(x, w, b), BF16).max()) > 1.0


# ---------------------------------------------------------------------------------------------------- timestep embedding
def ts_emul(t, dim, P=10000.0, mutant=None):
    half = dim // 2
    i = torch.arange(half, dtype=F32)
    den = float(max(half - 1, 1)) if mutant == "half_minus_1" else float(half)
    f = torch.exp(-torch.log(torch.tensor(P, dtype=F32)) * i / den)
    a = t.reshape(-1, 1).float() * f[None]
    if mutant == "bf16_argument":
        a = rbf(a)
    c, s = torch.cos(a), torch.sin(a)
    return (torch.cat([s, c], -1) if mutant == "swapped" else torch.cat([c, s], -1)).to(BF16)


def test_timestep_embedding_faithful_accepted_and_mutants_rejected():
    t = torch.tensor(RB.TS, dtype=F32)
    for dim in (2, 256, 258):
        y, b = RB.timestep_ref(t, dim)
        assert outside(ts_emul(t, dim), y, b) == 0, dim
    y, b = RB.timestep_ref(t, 256)
    for mutant in ("half_minus_1", "swapped", "bf16_argument"):
        assert outside(ts_emul(t, 256, mutant=mutant), y, b) > 0, mutant


# ---------------------------------------------------------------------------------------------------- row softmax
def softmax_emul(s, valid, scale, order=0, mutant=None):
    rows, cols = s.shape
    ok = torch.arange(cols)[None] < valid[:, None]
    ninf = torch.tensor(-math.inf)
    m = (s if mutant == "max_over_cols" else torch.where(ok, s, ninf)).max(-1, keepdim=True).values * scale
    if mutant == "unshifted":
        e = torch.where(ok, torch.exp(s * scale), torch.zeros(()))
        return (e * (1.0 / sum32(e, order))).to(F16)
    e = torch.where(ok, torch.exp(s * scale - m), torch.zeros(()))
    den = e[:, :(cols // 1024) * 1024] if mutant == "short_denominator" else e
    return (e * (1.0 / sum32(den, order))).to(F16)


@pytest.mark.parametrize("cls", RB.SOFTMAX_CLASSES)
def test_softmax_faithful_accepted(cls):
    for cols in (1, 4, 70, 257, 1020, 1024, 1025, 1028, 2052):
        for cb in (0, 4, 7, 1024):
            s = RB.softmax_scores(cls, 9, cols, f"sm.{cols}")
            valid = RB.valid_of(9, cols, cb)
            p, b = RB.softmax_ref(s, valid, 0.7)
            for o in ORDERS:
                assert outside(softmax_emul(s, valid, 0.7, o), p, b) == 0, (cls, cols, cb, o)


def test_softmax_mutants_rejected():
    # the row maximum over `cols`: the masked part of a causal row holds a score 100 above its visible ones, so the visible
    # exponentials all underflow
    s = RB.softmax_scores("flat", 8, 2052, "smm")
    s[:, 2000] += 100.0
    valid = RB.valid_of(8, 2052, 1024)
    p, b = RB.softmax_ref(s, valid, 1.0)
    assert outside(softmax_emul(s, valid, 1.0), p, b) == 0
    assert outside(softmax_emul(s, valid, 1.0, mutant="max_over_cols"), p, b) > 0
    valid = RB.valid_of(8, 2052, 0)
    s = RB.softmax_scores("flat", 8, 2052, "smm2")
    p, b = RB.softmax_ref(s, valid, 1.0)
    assert outside(softmax_emul(s, valid, 1.0, mutant="short_denominator"), p, b) > 0
    # no shift by the row maximum: on spread rows (scores over +-60, scale 2: exponents up to 120) the exponential overflows
    s = RB.softmax_scores("spread", 8, 2052, "smm3")
    p, b = RB.softmax_ref(s, valid, 2.0)
    assert outside(softmax_emul(s, valid, 2.0), p, b) == 0
    assert outside(softmax_emul(s, valid, 2.0, mutant="unshifted"), p, b) > 0


# ---------------------------------------------------------------------------------------------------- GroupNorm apply, the rest
def gn_emul(x, affine, silu, mutant=None):
    sc, sh = affine[:, 0][None], affine[:, 1][None]
    if mutant == "swapped":
        sc, sh = sh, sc
    t = x.float() * sc + sh
    return (silu32(t) if silu else t).to(F16)


def gn_operands(M, Cn, key):
    return U((M, Cn), key + ".x", 2.0).to(F16), torch.stack([1.0 + U((Cn,), key + ".sc", 0.5), U((Cn,), key + ".sh", 1.0)], 1).contiguous()


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_apply_faithful_accepted_and_swap_rejected(silu):
    for Cn in (8, 96, 2048):
        x, aff = gn_operands(23, Cn, f"gn.{Cn}")
        y, b = RB.gn_apply_ref(x, aff, silu)
        assert outside(gn_emul(x, aff, silu), y, b) == 0
        assert outside(gn_emul(x, aff, silu, mutant="swapped"), y, b) > 0


def test_euler_accepts_both_contractions():
    s, v = U((1027,), "eu.s"), U((1027,), "eu.v").to(BF16)
    dt = -0.0123
    y, b = RB.euler_ref(s, v, dt)
    two = s + v.float() * torch.tensor(dt, dtype=F32)
    fma = (s.double() + v.double() * float(torch.tensor(dt, dtype=F32))).float()
    assert outside(two, y, b) == 0 and outside(fma, y, b) == 0
    assert outside(s + rbf(v.float() * torch.tensor(dt, dtype=F32)), y, b) > 0         # the product rounded to bf16


def test_temporal_average_and_masked_mean_accept_fp32_sums():
    x = U((5 * 7, 72), "ta", 2.0).to(F16)
    for k, s in ((1, 1), (2, 2), (3, 2), (4, 3)):
        y, b = RB.temporal_avg_ref(x, 5, 7, k, s)
        x3 = x.float().reshape(5, 7, 72)
        t_out = (5 - 1) // s + 1
        acc = torch.zeros(t_out, 7, 72)
        for i in range(k):
            acc = acc + x3[(torch.arange(t_out) * s + i - (k - 1)).clamp(min=0)]
        assert outside((acc * torch.tensor(1.0 / k, dtype=F32)).to(F16).reshape(-1, 72), y, b) == 0
    xm = U((300, 257), "mm").to(BF16)
    mask = (torch.arange(300) < 117).int()
    xm[117:] = 1e30
    ref = RB.masked_mean_ref(xm, mask)
    sm, c = torch.zeros(257), torch.zeros(())
    for l in range(300):
        sm = sm + xm[l].float() * float(mask[l])
        c = c + float(mask[l])
    assert float(EB.ratio((sm / c).to(BF16)[None], ref, BF16).max()) <= 1.0
    assert float(EB.ratio((sm / 300.0).to(BF16)[None], ref, BF16).max()) > 1.0          # divided by L instead of the mask count


# ---------------------------------------------------------------------------------------------------- the measured mismatch shares
def test_mismatch_share_of_faithful_emulations(capsys):
    """Prints the largest share each faithful emulation reaches; rowwise_bounds.MEASURED_SHARE must not be below it (the cap is 4 x)."""
    worst = {"qknorm": (0.0, None), "silu_in": (0.0, None)}
    worst.update({f"ln.{cls}": (0.0, None) for cls in RB.LN_CLASSES})

    def rec(op, share, what):
        if share > worst[op][0]:
            worst[op] = (share, what)

    for cls in RB.LN_CLASSES:
        for D in RB.LN_DS:
            x = RB.data_rows(cls, 5, D, f"ln.{D}")
            shift, scale = _ln_mod(D, f"ln.{D}")
            weight = (1.0 + 0.6 * scale.float()).to(BF16)
            for mode, (a, m, aff) in {"shift+scale": (shift, scale, False), "scale": (None, scale, False), "shift": (shift, None, False),
                                      "neither": (None, None, False), "affine": (shift, weight, True)}.items():
                y, _ = RB.ln_ref(x, a, m, affine=aff)
                for o in ORDERS:
                    if x.numel() >= 512:                    # below that one element is more than the share being measured
                        rec(f"ln.{cls}", RB.mismatch_share(ln_emul(x, a, m, order=o, affine=aff), y, BF16), (cls, D, mode, o))
    for cls in RB.QK_CLASSES:
        for H in RB.QK_HEADS:
            for n_rows, n_rope in RB.QK_ROWS:
                key = f"qk.{H}.{n_rope}"
                _, x, w, _, _ = RB.qk_case(cls, H, n_rows, key)
                cos, sin = RB.rope_tables_independent(n_rows, key)
                y, _, amb, _ = RB.qknorm_ref(x, w, cos, sin, n_rope)
                for o in ORDERS:
                    if x.numel() >= 5120:
                        rec("qknorm", RB.mismatch_share(qk_emul(x, w, cos, sin, n_rope, order=o), y, BF16, amb), (cls, H, n_rope, o))
    for K in (256, 512, 520, 3080):
        x, w, b = RB.gemv_operands(4, 41, K, f"gemv.silu.{K}")
        x = RB.tie_free_for_silu(x)
        ref = EB.gemm_ref(RB.silu64(x).to(BF16), w, b)
        for o in ORDERS:
            rec("silu_in", RB.mismatch_share(gemv_emul(x, w, b, o, silu_in=True), ref.y, BF16), (K, o))
        bad = RB.mismatch_share(gemv_emul(x, w, b, 0, silu_in=True, mutant="silu_in_unrounded"), ref.y, BF16)
        assert bad > RB.mismatch_cap("silu_in", ref.y.numel()), (K, bad)
    with capsys.disabled():
        for op, (share, what) in worst.items():
            print(f"\nmismatch share of the faithful emulation, {op}: largest {share:.4f} at {what}; recorded {RB.MEASURED_SHARE[op]:.4f}, "
                  f"cap {4 * RB.MEASURED_SHARE[op]:.4f}")
    for op, (share, what) in worst.items():
        assert share <= RB.MEASURED_SHARE[op], (op, share, what)
        assert RB.MEASURED_SHARE[op] <= 2.0 * share + 1e-4, f"{op}: the recorded share {RB.MEASURED_SHARE[op]} is stale (measured {share})"
