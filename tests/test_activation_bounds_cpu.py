"""What tests/activation_bounds.py accepts and rejects, without a GPU: faithful fp32 emulations of gelu_tanh_f and silu_f pass every
bound, the specials table and every mismatch cap on every value set; each listed way an activation can be subtly wrong is rejected by
the check named for it.  test_measured_shares prints the mismatch shares recorded in activation_bounds.MEASURED_SHARE."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import activation_bounds as AB
from tests import rowwise_bounds as RB

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF16, F16]
FNS = ["gelu", "silu"]
TINY32 = 2.0 ** -126


# ---------------------------------------------------------------------------------------------------- the two 1-ulp instructions
def _moved(f, ulps):
    """f with every finite, non-zero result moved by `ulps` fp32 ulps (an instruction good to 1 ulp keeps 0 and inf)"""
    def g(a):
        r = f(a)
        m = torch.nextafter(r, torch.full_like(r, math.inf if ulps > 0 else -math.inf))
        return torch.where(torch.isfinite(r) & (r != 0) & torch.isfinite(m) & (m != 0), m, r)
    return g if ulps else f


def _ftz(v):
    return torch.where(v.abs() < TINY32, torch.copysign(torch.zeros_like(v), v), v)


def _flushing(f):
    """a unit that reads a subnormal operand as zero and returns zero for a subnormal result (v_exp_f32, v_rcp_f32)"""
    return lambda a: _ftz(f(_ftz(a)))


UNITS = {"exact": (torch.exp2, torch.reciprocal)}
UNITS.update({f"exp2{a:+d} rcp{b:+d}": (_moved(torch.exp2, a), _moved(torch.reciprocal, b)) for a in (1, -1) for b in (1, -1)})
UNITS["flushing units"] = (_flushing(torch.exp2), _flushing(torch.reciprocal))


def kernel_gelu(x, exp2=torch.exp2, rcp=torch.reciprocal):
    """gelu_tanh_f, operation by operation in fp32"""
    k0, k1 = torch.tensor(0.7978845608028654, dtype=F32), torch.tensor(0.044715, dtype=F32)
    u = k0 * (x + k1 * x * x * x)
    e = exp2(u * torch.tensor(2.8853900817779268, dtype=F32))
    t = 1.0 - 2.0 * rcp(e + 1.0)
    return 0.5 * x * (1.0 + t)


def kernel_silu(x, exp2=torch.exp2, rcp=torch.reciprocal):
    """silu_f: x * rcp(1 + __expf(-x)), __expf(a) = exp2(log2e * a)"""
    return x * rcp(1.0 + exp2(torch.tensor(1.4426950216293335, dtype=F32) * -x))      # 0x1.715476p+0


KERNEL = {"gelu": kernel_gelu, "silu": kernel_silu}
TORCH = {"gelu": lambda x: F.gelu(x, approximate="tanh"), "silu": F.silu}


def emulations(fn):
    em = {name: (lambda x, u=u: KERNEL[fn](x, *u)) for name, u in UNITS.items()}
    em["all flushed"] = lambda x: _ftz(KERNEL[fn](_ftz(x), *UNITS["flushing units"]))    # subnormal inputs and results flushed as well
    em["torch fp32"] = TORCH[fn]
    return em


def trunc_to(v32, dtype):
    """fp32 -> dtype by truncation (towards zero)"""
    r = v32.to(dtype)
    over = r.float().abs() > v32.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)


def outside(got, y64, bound):
    return int((RB.ratio(got, y64, bound) > 1.0).sum())


@pytest.fixture(scope="module")
def sets():
    s = {}
    for dt in DTYPES:
        x = AB.finite_values(dt)
        v, d, pre = AB.offset_set(dt)
        s[dt] = dict(x=x, pre=pre, xr=AB.rne(pre, dt), v=v, d=d)
        for fn in FNS:
            s[dt][fn] = AB.act_ref(fn, x, dt)
            s[dt][fn + ".off"] = AB.act_ref(fn, s[dt]["xr"], dt)
    return s


def shares_of(fn, dt, S, out_x, out_off):
    y, e32, _ = S[fn]
    core = AB.core_mask(y, e32, dt)
    yo, eo, _ = S[fn + ".off"]
    return {"exact": AB.mismatch_share(out_x, y, dt), "core": AB.mismatch_share(out_x, y, dt, ~core),
            "offset": AB.mismatch_share(out_off, yo, dt, ~AB.offset_window(S["v"], yo, eo, dt))}


# ---------------------------------------------------------------------------------------------------- the table of specials
def test_specials_are_torchs_fp32_results():
    x = torch.tensor([s for s, _ in AB.SPECIALS], dtype=F32)
    for fn in FNS:
        for f in (TORCH[fn], KERNEL[fn]):
            assert AB.specials_violations(f(x), x).numel() == 0, fn
    want = torch.tensor([w for _, w in AB.SPECIALS], dtype=F32)
    got = F.silu(x)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])
    assert torch.equal(torch.signbit(got[3:]), torch.signbit(want[3:]))
    # every NaN pattern of both formats is a NaN of the table, and an accumulating site's +0 for -0 is told apart from a lost sign
    for dt in DTYPES:
        v = AB.all_values(dt)
        sp = v[~torch.isfinite(v.float()) | (v.float() == 0)]
        assert sp.numel() == (256 if dt == BF16 else 2048) + 2
        for fn in FNS:
            assert AB.specials_violations(KERNEL[fn](sp.float()).to(dt), sp).numel() == 0
            acc = KERNEL[fn](sp.float() + 0.0).to(dt)
            assert AB.specials_violations(acc, sp).numel() == 1 and AB.specials_violations(acc, sp, accumulates=True).numel() == 0


def test_value_sets():
    for dt, n_fin in ((BF16, 65280), (F16, 63488)):
        assert AB.finite_values(dt).numel() == n_fin and torch.equal(AB.all_values(dt).view(torch.int16)[:3], torch.tensor([0, 1, 2], dtype=torch.int16))
        v, d, pre = AB.offset_set(dt)
        u = AB.ulp_out(v.double(), dt)
        off = (pre.double() - v.double()) / u
        assert set(off.abs().unique().tolist()) == {0.25, 0.375, 0.5} and v.numel() > 300000
        assert bool(torch.isfinite(AB.rne(pre, dt).float()).all())
        tie = off.abs() == 0.5
        # a tie rounds to the even neighbour: RNE and truncation differ on about half of them, and on every 3/8 offset away from zero
        assert 0.3 < float((AB.rne(pre, dt)[tie] != trunc_to(pre, dt)[tie]).float().mean()) < 0.7


def test_floor_cannot_hide_a_normal_result():
    """FLOOR is zero outside the two regions that can flush, and inside them it is the size of the values at stake"""
    for dt in DTYPES:
        x = AB.finite_values(dt)
        for fn in FNS:
            f = AB.floor_term(fn, x)
            on = f > 0
            assert bool(((x.double().abs() < 2.0 ** -124) | ((x.double() <= AB.SILU_FLOOR_FROM) & (fn == "silu")))[on].all())
            assert float(f.max()) <= AB.FLOOR == 2.0 ** -119
    # the SiLU overflow region: the true value is below FLOOR everywhere in it, and a normal bf16 number at its upper end
    x = AB.finite_values(BF16)
    reg = x.double() <= AB.SILU_FLOOR_FROM
    y = AB.silu64(x)[reg].abs()
    assert float(y.max()) < 87.5 * 2.0 ** -126 < AB.FLOOR and float(y.max()) > 2.0 ** -126


# ---------------------------------------------------------------------------------------------------- faithful emulations
@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_faithful_emulations_accepted(fn, dt, sets):
    S = sets[dt]
    y, _, bound = S[fn]
    yo, _, bo = S[fn + ".off"]
    sp = torch.tensor([s for s, _ in AB.SPECIALS], dtype=F32).to(dt)
    for name, f in emulations(fn).items():
        out, off = f(S["x"].float()).to(dt), f(S["xr"].float()).to(dt)
        assert bool(torch.isfinite(out.float()).all()), (name, "non-finite for a finite input")
        AB.check(out, y, bound, f"{fn} {AB.NAME[dt]} {name}")
        AB.check(off, yo, bo, f"{fn} {AB.NAME[dt]} {name} offset set")
        # the table's -inf row rests on rcp(1) = 1 exactly (1 + t = 0, inf * 0): a unit moved by an ulp THERE gives -inf * -2^-22 = +inf,
        # so the moved units are held to the bounds and caps only
        if name in ("exact", "flushing units", "torch fp32"):
            assert AB.specials_violations(f(sp.float()).to(dt), sp).numel() == 0, name
        for cls, share in shares_of(fn, dt, S, out, off).items():
            n = y.numel() if cls != "offset" else int(AB.offset_window(S["v"], yo, S[fn + ".off"][1], dt).sum())
            assert share <= AB.mismatch_cap(fn, dt, cls, n), (name, cls, share)


@pytest.mark.parametrize("fma", [False, True])
def test_gn_affine_act8_form_accepted(fma):
    """t = x sc + sh in fp32 (two roundings, or the FMA hipcc may contract them to), then silu_f, one rounding to fp16: inside
    rowwise_bounds.gn_apply_ref for every fp16 input (outputs beyond the fp16 range left out: they are not the activation's business)"""
    x = AB.finite_values(F16)[:, None]
    for sc, sh in ((1.0, 0.0), (1.0, -0.0), (1.5, -0.25), (-0.7, 3.0), (2.0 ** -10, 0.0), (0.37, 1e-3)):
        aff = torch.tensor([[sc, sh]], dtype=F32)
        t = (x.double() * aff[0, 0].double() + aff[0, 1].double()).float() if fma else x.float() * aff[0, 0] + aff[0, 1]
        for silu in (False, True):
            for name, u in UNITS.items():
                out = (kernel_silu(t, *u) if silu else t).to(F16)
                y, b = RB.gn_apply_ref(x, aff, silu)
                RB.check(out, y, b, f"gn_affine_act8 ({sc}, {sh}) silu {silu} fma {fma} {name}", skip=y.abs() > 65504.0)
        if sc == 1.0:                       # the identity affine: t is x exactly, the plain SiLU bound and caps hold (shift -0 keeps -0)
            y, e32, b = AB.act_ref("silu", x, F16)
            out = kernel_silu(t).to(F16)
            AB.check(out, y, b, "gn identity affine")
            assert AB.mismatch_share(out, y, F16, ~AB.core_mask(y, e32, F16)) <= AB.mismatch_cap("silu", F16, "core", y.numel())
            assert torch.equal(torch.signbit(t.to(F16)[x == 0]), torch.signbit(x[x == 0]) & (math.copysign(1.0, sh) < 0))


def test_measured_shares(sets, capsys):
    """prints the largest share each class reaches over the faithful emulations; MEASURED_SHARE must not be below it, nor stale"""
    lines, checks = [], []
    for fn in FNS:
        for dt in DTYPES:
            worst = {}
            for name, f in emulations(fn).items():
                S = sets[dt]
                for cls, share in shares_of(fn, dt, S, f(S["x"].float()).to(dt), f(S["xr"].float()).to(dt)).items():
                    if share >= worst.get(cls, (-1.0, None))[0]:
                        worst[cls] = (share, name)
            for cls, (share, name) in worst.items():
                key = f"{fn}.{AB.NAME[dt]}.{cls}"
                rec = AB.MEASURED_SHARE[key]
                lines.append(f"  {key:<18} largest {share:.5f} ({name}); recorded {rec:.5f}, cap {4 * rec:.5f}")
                checks.append((key, share, name, rec))
    with capsys.disabled():
        print("\nmismatch share of the faithful emulations:\n" + "\n".join(lines))
    for key, share, name, rec in checks:
        assert share <= rec, (key, share, name)
        assert rec <= 2.0 * share + 1e-4, f"{key}: the recorded share {rec} is stale (measured {share})"


# ---------------------------------------------------------------------------------------------------- mutants
def _table_gelu(x):
    """256 entries over [-8, 8] with linear interpolation; 0 below, x above"""
    n = 256
    h = 16.0 / (n - 1)
    knots = kernel_gelu(torch.arange(n, dtype=F32) * h - 8.0)
    p = ((x + 8.0) / h).clamp(0, n - 1 - 1e-3)
    i = p.floor().long()
    w = p - i.float()
    y = knots[i] * (1 - w) + knots[i + 1] * w
    return torch.where(x < -8.0, torch.zeros_like(x), torch.where(x > 8.0, x, y))


def _tanh_em1(x):
    u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
    e = torch.exp(2.0 * u)
    return 0.5 * x * (1.0 + (e - 1.0) / (e + 1.0))


BOUND_MUTANTS = {
    "gelu": {"erf": lambda x: F.gelu(x), "tail clamped below -4": lambda x: torch.where(x < -4.0, torch.zeros_like(x), kernel_gelu(x)),
             "table": _table_gelu},
    "silu": {"gelu for silu": kernel_gelu},
}
NONFINITE_MUTANTS = {"gelu": {"tanh as (e - 1) / (e + 1)": _tanh_em1}, "silu": {"sigmoid as e^x / (1 + e^x)": lambda x: x * (torch.exp(x) / (1.0 + torch.exp(x)))}}


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_mutants_rejected(fn, dt, sets):
    S = sets[dt]
    x32 = S["x"].float()
    y, e32, bound = S[fn]
    yo, _, bo = S[fn + ".off"]
    k = KERNEL[fn]
    # by the bound
    for name, f in BOUND_MUTANTS[fn].items():
        assert outside(f(x32).to(dt), y, bound) > 0, name
    # by "a finite input gives a finite output"
    for name, f in NONFINITE_MUTANTS[fn].items():
        out = f(x32).to(dt)
        assert not bool(torch.isfinite(out.float()).all()), name
    # by the offset-set share: the activation of the unrounded sum, truncation in the pre-rounding and at the store
    out_w = ~AB.offset_window(S["v"], yo, S[fn + ".off"][1], dt)
    n = int((~out_w).sum())
    cap = AB.mismatch_cap(fn, dt, "offset", n)
    unrounded = AB.mismatch_share(k(S["pre"]).to(dt), yo, dt, out_w)
    assert unrounded >= 0.1 and unrounded > cap, unrounded
    pre_trunc = AB.mismatch_share(k(trunc_to(S["pre"], dt).float()).to(dt), yo, dt, out_w)
    store_trunc = AB.mismatch_share(trunc_to(k(S["xr"].float()), dt), yo, dt, out_w)
    print(f"{fn} {AB.NAME[dt]}: offset-set share in the window: unrounded {unrounded:.3f}, truncated pre-rounding {pre_trunc:.3f}, truncated store {store_trunc:.3f}")
    assert pre_trunc >= 0.1 and store_trunc >= 0.1, (pre_trunc, store_trunc)
    tie = ((S["pre"].double() - S["v"].double()).abs() / AB.ulp_out(S["v"].double(), dt)) == 0.5
    tie_share = AB.mismatch_share(k(trunc_to(S["pre"], dt).float()).to(dt)[tie], yo[tie], dt, out_w[tie])
    assert tie_share > 0.2, tie_share                          # the tie cases alone: about half of them round the other way
    # ... and the store's truncation also by the core share of the exact set
    core = AB.core_mask(y, e32, dt)
    assert AB.mismatch_share(trunc_to(k(x32), dt), y, dt, ~core) > AB.mismatch_cap(fn, dt, "core", y.numel())
    # by the specials table (and by nothing else: the bound holds for them)
    sp = torch.tensor([s for s, _ in AB.SPECIALS], dtype=F32).to(dt)
    lost_sign = (k(sp.float()) + 0.0).to(dt)
    assert AB.specials_violations(lost_sign, sp).tolist() == [3]
    for z in (-0.0, 0.0):
        minus_inf = torch.where(sp.float() == -math.inf, torch.full((), z), k(sp.float())).to(dt)
        assert AB.specials_violations(minus_inf, sp).tolist() == [1]
    assert outside((k(x32) + 0.0).to(dt), y, bound) == 0
