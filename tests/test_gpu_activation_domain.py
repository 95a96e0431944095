"""GPU: gelu_tanh_f and silu_f (csrc/hv_common.hpp) on every 16-bit input at every call site, against the fp64 references, bounds,
specials table and mismatch caps of tests/activation_bounds.py (what those accept and reject: tests/test_activation_bounds_cpu.py).

The contract.  Every site applies the function to a 16-bit value - the ROUNDED pre-activation (round to nearest even of the fp32 sum) -
and rounds the fp32 result once to the output type.  Outside GELU's negative tail the result is within one ulp of the fp64 value of
that function (the "within 1 ulp" of tests/test_gpu_gemm_conv_edges.py), and on all but a few in ten thousand inputs it is the
correctly rounded value.  Inside the tail - x < -4 for bf16, x < -3.5 for fp16, where 1 + tanh(u) cancels - the error is ABSOLUTE:
|x| delta / 2 with delta = (6 (1 - s) + |tanh u|) 2^-24 <= 7 * 2^-24, up to a few hundred ulp of a value below 1e-8; torch's own fp32
gelu has the same property.  SiLU has no tail; below x = -87.33 its result may be -0 for a true value of up to 87.4 * 2^-126 (FLOOR =
128 * 2^-126 there, FLUSH = 2^-126 for |x| < 2^-124, zero elsewhere).  +inf -> +inf, -inf -> NaN, NaN -> NaN, a zero keeps its sign where
the site lets a -0 through (a site that accumulates turns -0 into +0 before or after the function: +0 + -0 = +0).

Sites, and how every value reaches them exactly (an inf or NaN is only ever multiplied by 1, zeros only by zeros):
    hv_gemm_bf16 epilogue     B1 (values down the rows: A[m][0] = V[m], W[n][0] = 1), B2 and B3 (across the columns: W[n][0] = V[n],
                              A[m][0] = 1; K = 64 and 192), each also by the bias route (A = 0, bias = V; B1 in 512 launches of N = 128);
                              n_split in the middle with the other function behind it; gate + residual over the whole set; the offset
                              set on B1 - B3 (A[m][1] = d, W[n][1] = 1 or the transpose), bit-equal to the site's own table at RNE(v + d)
    hv_gemm_fp8 (Q)           zero e4m3 operands, bias = V, row scale 1.  The offset set is left out: it would need v = hi + lo / 16 from
                              two e4m3 products, and the fp8 MFMA's reduction is not known to be exact (tests/error_bounds.py)
    hv_linear_smallm_bf16     silu_out (bias = V, x = 0); silu_in (the finite values through an identity W, K = N = 512, M = 4, 32 launches;
                              the five specials one per launch); both flags (bit-equal to the silu_out table at the silu_in result)
    hv_groupnorm_apply_f16    every fp16 pattern, affine (1, +0) and (1, -0) (only the second lets -0 through: -0 * 1 + +0 = +0), SiLU on
                              and off, as [8192, 8] and [32, 2048]; SiLU off returns x * 1 + shift bit for bit
    hv_conv3d_cout4_f16       the finite fp16 values in channels 0..2 of 131 x 162 voxels, Cin = 32, weights selecting channel c at the
                              tap that reads the voxel itself: the same bits as hv_groupnorm_apply_f16 (-0 as +0: the taps are summed)
    hv_quant_rows_fp8         (related sweep) rows with maximum 448 * 2^j, j in {0, -3, 100}, every bf16 value below: codes bit-equal to
                              torch's float8_e4m3fn cast of v * 2^-j, scales bit-equal to 2^j

Every operand sits in NaN-poisoned memory, every output in a sentinel-guarded buffer, every launch is repeated and gives the same bits.
All sites of one function and dtype give the same bits for the same pre-activation (test_sibling_sites_agree).  test_zz_ratio_report
prints the largest error-to-bound ratio per site (each must lie in (0.05, 1]) and what the tail alone reaches.

Measured on an MI355X (this file's own run; ratio = largest |got - f64| / bound, tail = the same inside GELU's tail alone, shares = outputs
whose bits differ from RNE(fp64), oracle = outputs differing from oracle.dit_ref's fp32 formula rounded to the output type):

    site                                   function   ratio   tail    share all finite   outside tails   offset window   oracle
    B1, B2, B3 (both routes), Q            gelu       0.500   0.447   0.00259 (169)      0.00002 (1)     0.00041 (4)     31 of 65,280
    B1, B2, B3 (both routes), Q, smallm    silu       0.578   -       0.00032 (21)       0.00003 (2)     0.00074 (8)     4 of 65,280
    gn_apply (both shapes, shifts), cout4  silu       0.500   -       0 of 63,488        0               -               1 of 63,488

Every site of a row has the same bits.  The tail uses 0.447 of |x| delta / 2, i.e. the hardware's 1 + t is off by 3.1 * 2^-24 at most
against the derived 7 * 2^-24; 168 of GELU's 169 differing inputs lie in it (as activation_bounds.tail_mask draws it).  SiLU's 21: 20 where
FLOOR applies - the 17 inputs below -88.72 (-0 for a true value of up to 22.6 * 2^-126) and the three in (-88.72, -87.33], whose reciprocal
v_rcp_f32 flushes - and one next to a rounding tie.  No site lost a subnormal operand or result elsewhere: the bf16 MFMA, the conversions
and the stores keep them.  No defect was found."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402
from tests import activation_bounds as AB  # noqa: E402
from tests.guarded_memory import Guarded, GuardedBytes, GuardedFlat, Poisoned, bits, poisoned_vec, same_bits  # noqa: E402
from tests.test_gpu_gemm_conv_edges import gemm_path  # noqa: E402

DEV = "cuda"
E = R.Prec(True)
BF16, F16, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
REPORT = {}                # (site, fn) -> dict(ratio, tail, exact, core, offset, oracle)
TABLES = {}                # (site, fn) -> the site's output for every 16-bit pattern, in bit order (CPU)
ORACLE = {"gelu": lambda x: R.gelu_tanh(x, R.FP32), "silu": lambda x: F.silu(x)}       # oracle.dit_ref's fp32 formulas, before its rounding


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def V():
    from hunyuanvideo_efficiency_amd import vae_ops, _lib
    _lib.load()
    return vae_ops


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 53, DEV) * (scale * math.sqrt(3.0))


def act_code(ops, fn):
    return ops.ACT_GELU_TANH if fn == "gelu" else ops.ACT_SILU


def same_bits_nan(a, b):
    """the same bits wherever neither is NaN, and NaN where the other is"""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    return torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def plus_zero(t):
    """-0 -> +0 (what a sum with +0 does), every other bit kept"""
    return torch.where(t == 0, torch.zeros_like(t), t)


def evaluate(site, fn, dt, pre, got, accumulates):
    """checks 1 - 4 and 6 of one site on the pre-activations `pre` (16-bit, specials included) and its outputs `got`"""
    pre, got = pre.cpu().reshape(-1), got.cpu().reshape(-1)
    what = f"{site} {fn}"
    fin = torch.isfinite(pre.float())
    x, g = pre[fin], got[fin]
    nonfin = ~torch.isfinite(g.float())
    assert not bool(nonfin.any()), f"{what}: non-finite outputs {g[nonfin][:8].tolist()} for the finite inputs {x[nonfin][:8].tolist()}"
    y, e32, bound = AB.act_ref(fn, x, dt)
    r = AB.ratio(g, y, bound)
    worst = AB.check(g, y, bound, what)
    tail = AB.tail_mask(fn, x, dt)
    bad = AB.specials_violations(got, pre, accumulates)
    assert bad.numel() == 0, f"{what}: the specials table is broken: {pre[bad][:8].tolist()} -> {got[bad][:8].tolist()}"
    core = AB.core_mask(y, e32, dt)
    miss = g != y.to(dt)
    rep = dict(ratio=worst, tail=float(r[tail].max()) if bool(tail.any()) else 0.0,
               exact=AB.mismatch_share(g, y, dt), core=AB.mismatch_share(g, y, dt, ~core),
               oracle=int((ORACLE[fn](x.float()).to(dt) != g).sum()))
    REPORT[(site, fn)] = rep
    print(f"{what}: ratio {worst:.3f} (tail {rep['tail']:.3f}); differs in bits from RNE(fp64) on {rep['exact']:.5f} of the finite inputs "
          f"({int(miss.sum())}: {int((miss & tail).sum())} in the tail, {int((miss & (AB.floor_term(fn, x) > 0)).sum())} where FLOOR applies, "
          f"{int((miss & core).sum())} outside both), {rep['core']:.5f} outside the tails; from the oracle's fp32 formula on {rep['oracle']} of {x.numel()}")
    for cls, n in (("exact", x.numel()), ("core", int(core.sum()))):
        cap = AB.mismatch_cap(fn, dt, cls, n)
        assert rep[cls] <= cap, f"{what}: mismatch share {rep[cls]:.5f} of class {cls} above its cap {cap:.5f}"
    return rep


def evaluate_offsets(site, fn, dt, pre32, v, got, lut):
    """the offset set: within the bound of act(RNE(v + d)), the mismatch share inside the window within its cap, and bit-equal to the
    site's own table at RNE(v + d) - the activation saw the rounded pre-activation"""
    xr = AB.rne(pre32, dt)
    got = got.cpu().reshape(-1)
    y, e32, bound = AB.act_ref(fn, xr, dt)
    AB.check(got, y, bound, f"{site} {fn} offset set")
    win = AB.offset_window(v, y, e32, dt)
    share = AB.mismatch_share(got, y, dt, ~win)
    cap = AB.mismatch_cap(fn, dt, "offset", int(win.sum()))
    REPORT[(site, fn)]["offset"] = share
    print(f"{site} {fn}: offset set: differs from act(RNE(v + d)) on {share:.5f} of {int(win.sum())} window elements (cap {cap:.5f})")
    assert share <= cap, f"{site} {fn}: offset-set mismatch share {share:.5f} above {cap:.5f}: the activation does not see the rounded value"
    idx = bits(xr).long() & 0xFFFF
    assert torch.equal(bits(plus_zero(lut[idx])), bits(plus_zero(got))), f"{site} {fn}: act(v + d) is not the site's own act(RNE(v + d))"


# ---------------------------------------------------------------------------------------------------- hv_gemm_bf16 / hv_gemm_fp8
GEMM_SHAPES = {"B1": (65536, 8, 64), "B2": (3, 65536, 64), "B3": (3, 65536, 192), "Q": (3, 65536, 384)}


def _gemm_operands(path, v, d=None):
    """(a, w) with v (and the second addend d) placed so that output [m, n] is v[m] (B1) or v[n] (B2, B3), everything else zero"""
    n_v = v.numel()
    if path == "B1":
        M, N, K = n_v, 8, 64
        a, w = torch.zeros(M, K, dtype=BF16, device=DEV), torch.zeros(N, K, dtype=BF16, device=DEV)
        a[:, 0], w[:, 0] = v, 1.0
        if d is not None:
            a[:, 1], w[:, 1] = d, 1.0
    else:
        M, N, K = 3, n_v, GEMM_SHAPES[path][2]
        a, w = torch.zeros(M, K, dtype=BF16, device=DEV), torch.zeros(N, K, dtype=BF16, device=DEV)
        a[:, 0], w[:, 0] = 1.0, v
        if d is not None:
            a[:, 1], w[:, 1] = 1.0, d
    assert gemm_path("bf16", N, K) == path
    return a, w


def _run_gemm(ops, path, a, w, what, **kw):
    """one guarded launch, repeated; returns the [n_v] values (all 8 columns of B1 / all 3 rows of B2, B3 agree)"""
    M, N = a.shape[0], w.shape[0]
    A, W = Poisoned(a, 3, 5, 24), Poisoned(w, 2, 7, 40)
    o = Guarded(M, N, BF16, c0=8)
    ops.gemm(A.view, W.view, None, out=o.view, **kw)
    assert o.intact() and A.intact() and W.intact(), f"{what}: a store outside the output"
    y = o.view.clone()
    ops.gemm(A.view, W.view, None, out=o.view, **kw)
    assert same_bits(o.view, y), f"{what}: a second launch differs"
    if path == "B1":
        assert bool((bits(y) == bits(y)[:, :1]).all()), f"{what}: the columns of a row differ"
        return y[:, 0].cpu()
    assert bool((bits(y) == bits(y)[:1]).all()), f"{what}: the rows of a column differ"
    return y[0].cpu()


def gemm_table(ops, path, fn, route):
    key = (f"{path}.{route}", fn)
    if key in TABLES:
        return TABLES[key]
    vals = AB.all_bf16().to(DEV)
    act = act_code(ops, fn)
    what = f"{path} {route} route {fn}"
    if route == "A":
        a, w = _gemm_operands(path, vals)
        y = _run_gemm(ops, path, a, w, what, act=act)
    elif path == "B1":                  # N <= 128: 512 launches of one row, 128 values each
        assert gemm_path("bf16", 128, 64) == "B1"
        a, w = torch.zeros(1, 64, dtype=BF16, device=DEV), torch.zeros(128, 64, dtype=BF16, device=DEV)
        bias = poisoned_vec(vals)
        o = Guarded(512, 128, BF16, c0=8)
        for rep in range(2):
            for i in range(512):
                ops.gemm(a, w, bias[i * 128:(i + 1) * 128], out=o.view[i:i + 1], act=act)
            if rep == 0:
                y = o.view.clone()
        assert o.intact() and same_bits(o.view, y), f"{what}: a store outside the output, or a second launch differs"
        y = y.reshape(-1).cpu()
    else:
        M, N, K = GEMM_SHAPES[path]
        bias = poisoned_vec(vals)
        o = Guarded(M, N, BF16, c0=8)
        if path == "Q":
            z8 = lambda r: torch.zeros(r, K, dtype=torch.uint8, device=DEV).view(FP8)           # noqa: E731
            A, W = Poisoned(z8(M), 3, 5, 32), Poisoned(z8(N), 2, 7, 48)
            asc, ws = poisoned_vec(torch.ones(M, dtype=F32, device=DEV)), torch.ones(1, dtype=BF16, device=DEV)
            run = lambda: ops.gemm_fp8(A.view, asc, W.view, ws, bias, out=o.view, act=act)      # noqa: E731
        else:
            assert gemm_path("bf16", N, K) == path
            A, W = Poisoned(torch.zeros(M, K, dtype=BF16, device=DEV), 3, 5, 24), Poisoned(torch.zeros(N, K, dtype=BF16, device=DEV), 2, 7, 40)
            run = lambda: ops.gemm(A.view, W.view, bias, out=o.view, act=act)                   # noqa: E731
        run()
        assert o.intact() and A.intact() and W.intact(), f"{what}: a store outside the output"
        y = o.view.clone()
        run()
        assert same_bits(o.view, y) and bool((bits(y) == bits(y)[:1]).all()), f"{what}: a second launch, or the rows of a column, differ"
        y = y[0].cpu()
    TABLES[key] = y
    return y


GEMM_SITES = [("B1", "A"), ("B1", "bias"), ("B2", "A"), ("B2", "bias"), ("B3", "A"), ("B3", "bias"), ("Q", "bias")]


@pytest.mark.parametrize("fn", ["gelu", "silu"])
@pytest.mark.parametrize("path,route", GEMM_SITES, ids=[f"{p}-{r}" for p, r in GEMM_SITES])
def test_gemm_epilogue_every_value(ops, path, route, fn):
    """the accumulator starts at +0, so a -0 value arrives as +0 (accumulates=True)"""
    evaluate(f"{path}.{route}", fn, BF16, AB.all_bf16(), gemm_table(ops, path, fn, route), accumulates=True)


@pytest.mark.parametrize("fn", ["gelu", "silu"])
@pytest.mark.parametrize("path", ["B1", "B2", "B3"])
def test_gemm_epilogue_offset_set(ops, path, fn):
    v, d, pre32 = AB.offset_set(BF16)
    pad = (-v.numel()) % 8
    vp, dp = torch.cat([v, torch.zeros(pad, dtype=BF16)]), torch.cat([d, torch.zeros(pad, dtype=BF16)])
    a, w = _gemm_operands(path, vp.to(DEV), dp.to(DEV))
    got = _run_gemm(ops, path, a, w, f"{path} offset set {fn}", act=act_code(ops, fn))[:v.numel()]
    lut = gemm_table(ops, path, fn, "A")
    if (f"{path}.A", fn) not in REPORT:
        evaluate(f"{path}.A", fn, BF16, AB.all_bf16(), lut, accumulates=True)
    evaluate_offsets(f"{path}.A", fn, BF16, pre32, v, got, lut)


def test_gemm_split_applies_the_other_function_behind_n_split(ops):
    """n_split in the middle of the value set: act0 in front of it, act1 behind (the epilogue's `second` branch), both orders"""
    a, w = _gemm_operands("B2", AB.all_bf16().to(DEV))
    A, W = Poisoned(a, 3, 5, 24), Poisoned(w, 2, 7, 40)
    ns = 32768
    for f0, f1 in (("gelu", "silu"), ("silu", "gelu")):
        o0, o1 = Guarded(3, ns, BF16, c0=0), Guarded(3, 65536 - ns, BF16, c0=24)
        for _ in range(2):
            ops.gemm(A.view, W.view, None, out=o0.view, act=act_code(ops, f0), n_split=ns, out1=o1.view, act1=act_code(ops, f1))
            assert o0.intact() and o1.intact()
            assert same_bits_nan(o0.view[0], gemm_table(ops, "B2", f0, "A")[:ns]), f"{f0} in front of n_split"
            assert same_bits_nan(o1.view[0], gemm_table(ops, "B2", f1, "A")[ns:]), f"{f1} behind n_split"
    assert A.intact() and W.intact()


@pytest.mark.parametrize("fn", ["gelu", "silu"])
def test_gemm_gate_residual_on_the_activation(ops, fn):
    """out = bf16(res + bf16(bf16(act) * gate)): the oracle's gate_residual on the plain activation output of the same kernel"""
    N = 65536
    a, w = _gemm_operands("B2", AB.all_bf16().to(DEV))
    A, W = Poisoned(a, 3, 5, 24), Poisoned(w, 2, 7, 40)
    gate, res = poisoned_vec(U((N,), "act.gate", 0.5).to(BF16)), U((3, N), "act.res").to(BF16)
    assert bool((gate != 0).all())
    Rs = Poisoned(res, 1, 4, 16)
    o = Guarded(3, N, BF16, c0=8)
    plain = gemm_table(ops, "B2", fn, "A").to(DEV).float().expand(3, N)
    want = R.gate_residual(res.float()[None], plain[None], gate.float()[None], E)[0].to(BF16)
    for _ in range(2):
        ops.gemm(A.view, W.view, None, out=o.view, act=act_code(ops, fn), gate=gate, res=Rs.view)
        assert o.intact() and Rs.intact() and A.intact() and W.intact()
        assert same_bits_nan(o.view, want), f"gate + residual behind {fn}"


# ---------------------------------------------------------------------------------------------------- hv_linear_smallm_bf16
def smallm_out_table(ops):
    key = ("smallm.silu_out", "silu")
    if key not in TABLES:
        N, K = 65536, 8
        X, W = Poisoned(torch.zeros(3, K, dtype=BF16, device=DEV), 3, 5, 24), Poisoned(torch.zeros(N, K, dtype=BF16, device=DEV), 2, 7, 0)
        bias = poisoned_vec(AB.all_bf16().to(DEV))
        o = Guarded(3, N, BF16, c0=8)
        ops.linear_smallm(X.view, W.view, bias, silu_out=True, out=o.view)
        assert o.intact() and X.intact() and W.intact()
        y = o.view.clone()
        ops.linear_smallm(X.view, W.view, bias, silu_out=True, out=o.view)
        assert same_bits(o.view, y) and bool((bits(y) == bits(y)[:1]).all())
        TABLES[key] = y[0].cpu()
    return TABLES[key]


def test_smallm_silu_out_every_value(ops):
    evaluate("smallm.silu_out", "silu", BF16, AB.all_bf16(), smallm_out_table(ops), accumulates=True)


def _smallm_in(ops, both):
    """the 65,280 finite values through an identity W: out[m][n] = bf16(silu(x[m][n])) (+ exact zeros), 2,048 per launch"""
    fv = AB.finite_values(BF16)
    x = torch.cat([fv, torch.zeros(65536 - fv.numel(), dtype=BF16)]).reshape(32, 4, 512).to(DEV)
    W = Poisoned(torch.eye(512, dtype=BF16, device=DEV), 2, 7, 0)
    o = Guarded(128, 512, BF16, c0=8)
    for rep in range(2):
        for i in range(32):
            X = Poisoned(x[i], 3, 5, 24)
            ops.linear_smallm(X.view, W.view, None, silu_in=True, silu_out=both, out=o.view[4 * i:4 * i + 4])
            assert X.intact()
        if rep == 0:
            y = o.view.clone()
    assert o.intact() and W.intact() and same_bits(o.view, y), "smallm silu_in: a store outside the output, or a second launch differs"
    return fv, y.reshape(-1)[:fv.numel()].cpu()


def test_smallm_silu_in_every_finite_value_and_both_flags(ops):
    fv, got = _smallm_in(ops, False)
    TABLES[("smallm.silu_in", "silu")] = (fv, got)
    evaluate("smallm.silu_in", "silu", BF16, fv, got, accumulates=True)              # the products are summed: a -0 result leaves as +0
    # both flags: silu_out of the bf16 sum, which is bf16(silu(x)) exactly: the silu_out table at that value
    _, both = _smallm_in(ops, True)
    lut = smallm_out_table(ops)
    assert torch.equal(bits(plus_zero(lut[bits(got).long() & 0xFFFF])), bits(plus_zero(both))), "silu_in + silu_out is not silu_out(bf16(silu(x)))"


def test_smallm_silu_in_specials(ops):
    """one special per launch (K = N = 8, M = 1, identity W), so that a NaN cannot spread along a row: only column 0 holds the value"""
    W = torch.eye(8, dtype=BF16, device=DEV)
    sp = torch.tensor([s for s, _ in AB.SPECIALS], dtype=BF16)
    got = []
    for s in sp.tolist():
        x = torch.zeros(1, 8, dtype=BF16, device=DEV)
        x[0, 0] = s
        out = ops.linear_smallm(x, W, None, silu_in=True)
        assert same_bits(out, ops.linear_smallm(x, W, None, silu_in=True))
        got.append(out[0, 0].cpu())
    bad = AB.specials_violations(torch.stack(got), sp, accumulates=True)
    assert bad.numel() == 0, (sp[bad].tolist(), torch.stack(got)[bad].tolist())


# ---------------------------------------------------------------------------------------------------- hv_groupnorm_apply_f16, hv_conv3d_cout4_f16
def _gn_run(V, x2d, shift, silu):
    C = x2d.shape[1]
    aff = torch.tensor([1.0, shift], dtype=F32, device=DEV).expand(C, 2).contiguous()
    X = Poisoned(x2d, 2, 6, 40)
    o = Guarded(x2d.shape[0], C, F16, c0=8)
    V.groupnorm_apply(X.view, aff, silu, out=o.view)
    assert o.intact() and X.intact(), "groupnorm_apply: a store outside the output"
    y = o.view.clone()
    V.groupnorm_apply(X.view, aff, silu, out=o.view)
    assert same_bits(o.view, y), "groupnorm_apply: a second launch differs"
    return y.reshape(-1).cpu()


@pytest.mark.parametrize("shift", [0.0, -0.0], ids=["shift+0", "shift-0"])
def test_groupnorm_apply_every_value(V, shift):
    vals = AB.all_fp16()
    t = (vals.float() * 1.0 + torch.tensor(shift, dtype=F32)).to(F16)          # the pre-activation: x itself, but -0 + +0 = +0
    neg_shift = math.copysign(1.0, shift) < 0
    for silu in (False, True):
        a, b = _gn_run(V, vals.to(DEV).reshape(8192, 8), shift, silu), _gn_run(V, vals.to(DEV).reshape(32, 2048), shift, silu)
        assert same_bits(a, b), f"groupnorm_apply silu {silu}: [8192, 8] and [32, 2048] give other bits"
        if not silu:
            assert same_bits_nan(a, t), "groupnorm_apply without SiLU does not return x * 1 + shift bit for bit"
            fin = torch.isfinite(vals.float())
            if not neg_shift:                      # -0 * 1 + +0 = +0: the one finite input an affine (1, +0) does not return
                fin = fin & ~((vals == 0) & torch.signbit(vals))
            assert torch.equal(bits(a)[fin], bits(vals)[fin]), "groupnorm_apply without SiLU changed a finite input"
        else:
            site = "gn_apply" + (".shift-0" if neg_shift else "")
            TABLES[(site, "silu")] = a
            evaluate(site, "silu", F16, t, a, accumulates=False)


def test_conv_cout4_has_the_bits_of_groupnorm_apply(V):
    """the header's claim: hv_conv3d_cout4_f16 normalises with "the arithmetic of hv_groupnorm_apply_f16".  Weights that pick channel c at
    the tap reading the voxel itself (kt = 2: the causal conv's last tap in time, kh = kw = 1) make out[v][c] = 0 + silu16(x[v][c]) + zeros"""
    T, H, W_, cin, cout = 1, 131, 162, 32, 3
    M = T * H * W_
    fv = AB.finite_values(F16)
    assert M * 3 >= fv.numel()
    x = torch.zeros(M, cin, dtype=F16, device=DEV)
    x[:, :3] = torch.cat([fv, torch.zeros(M * 3 - fv.numel(), dtype=F16)]).reshape(M, 3).to(DEV)
    aff = torch.tensor([1.0, 0.0], dtype=F32, device=DEV).expand(cin, 2).contiguous()
    w = torch.zeros(cout, cin, 3, 3, 3, dtype=F16, device=DEV)
    for c in range(cout):
        w[c, c, 2, 1, 1] = 1.0
    wf, bias = V.cout4_weight_fragments(w), poisoned_vec(torch.zeros(8, dtype=F16, device=DEV))
    X = Poisoned(x, 2, 6, 40)
    o = Guarded(M, 8, F16, c0=8)
    V.conv_cout4(X.view, aff, True, wf, bias, T, H, W_, cin, cout, out=o.view)
    assert o.intact() and X.intact(), "conv_cout4: a store outside the output"
    y = o.view.clone()
    V.conv_cout4(X.view, aff, True, wf, bias, T, H, W_, cin, cout, out=o.view)
    assert same_bits(o.view, y), "conv_cout4: a second launch differs"
    assert not bool(bits(y[:, 3:]).any()), "conv_cout4: columns behind Cout are not zero"
    got = y[:, :3].reshape(-1)[:fv.numel()].cpu()
    gn = V.groupnorm_apply(x, aff, True)[:, :3].reshape(-1)[:fv.numel()].cpu()
    TABLES[("cout4", "silu")] = (fv, got)
    diff = bits(plus_zero(gn)) != bits(plus_zero(got))
    assert not bool(diff.any()), f"conv_cout4 differs from groupnorm_apply on {int(diff.sum())} values, first {fv[diff][:8].tolist()}: {got[diff][:8].tolist()} vs {gn[diff][:8].tolist()}"
    evaluate("cout4", "silu", F16, fv, got, accumulates=True)


# ---------------------------------------------------------------------------------------------------- check 5: sibling sites
def test_sibling_sites_agree(ops, V):
    """all sites of one function and dtype give identical bits for identical pre-activations: B1 = B2 = B3 (both routes) = Q, and for
    SiLU = smallm silu_out = smallm silu_in (finite values; a zero result as +0); gn_apply = cout4 is asserted in its own test"""
    for fn in ("gelu", "silu"):
        first = gemm_table(ops, "B1", fn, "A")
        for path, route in GEMM_SITES[1:]:
            other = gemm_table(ops, path, fn, route)
            diff = bits(first) != bits(other)
            assert same_bits_nan(first, other), f"{fn}: B1.A and {path}.{route} differ on {AB.all_bf16()[diff & ~torch.isnan(first.float())][:8].tolist()}"
    ref = gemm_table(ops, "B1", "silu", "A")
    assert same_bits_nan(ref, smallm_out_table(ops)), "silu: the GEMM epilogue and smallm silu_out differ"
    fv, got = TABLES.get(("smallm.silu_in", "silu")) or _smallm_in(ops, False)
    fin = torch.isfinite(AB.all_bf16().float())
    assert torch.equal(bits(plus_zero(ref[fin])), bits(plus_zero(got))), "silu: the GEMM epilogue and smallm silu_in differ"


# ---------------------------------------------------------------------------------------------------- hv_quant_rows_fp8
@pytest.mark.parametrize("j", [0, -3, 100])
def test_quant_rows_fp8_every_value_below_a_power_of_two_scale(ops, j):
    """a row maximum of 448 * 2^j makes the row scale 448 * 2^j * fl(1 / 448) = 2^j exactly (7 * fl(1 / 7) = 1 + 3 * 2^-26 rounds to 1) and
    the division exact: the codes are the e4m3 rounding of v * 2^-j alone"""
    top = 448.0 * 2.0 ** j
    fv = AB.finite_values(BF16)
    vals = fv[fv.float().abs() <= top]
    K = 512
    rows = -(-vals.numel() // (K - 1))
    x = torch.zeros(rows, K, dtype=BF16)
    x[:, 1:] = torch.cat([vals, torch.zeros(rows * (K - 1) - vals.numel(), dtype=BF16)]).reshape(rows, K - 1)
    x[:, 0] = top
    assert float(x[0, 0]) == top
    X = Poisoned(x.to(DEV), 3, 5, 8)
    q, s = GuardedBytes(rows, K, K + 16), GuardedFlat(rows, F32)
    ops.quant_rows_fp8(X.view, out_q=q.view, out_scale=s.view)
    assert q.intact() and s.intact() and X.intact()
    q0 = q.view.clone()
    ops.quant_rows_fp8(X.view, out_q=q.view, out_scale=s.view)
    assert same_bits(q.view, q0)
    assert same_bits(s.view.cpu(), torch.full((rows,), 2.0 ** j, dtype=F32)), f"row scales {s.view[:4].tolist()} are not 2^{j}"
    want = (x.float() * 2.0 ** -j).to(FP8)
    diff = bits(q0.cpu()) != bits(want)
    assert not bool(diff.any()), f"j = {j}: {int(diff.sum())} codes differ from torch's e4m3 cast, first at {x[diff][:8].tolist()}: {q0.cpu()[diff][:8].float().tolist()}"


# ---------------------------------------------------------------------------------------------------- the report
def test_zz_ratio_report():
    """largest error-to-bound ratio per site over this module's cases (run after them): each in (0.05, 1]; the tail's own ratio shows
    how much of delta the hardware uses"""
    lines = [f"  {s + ' ' + fn:<26} ratio {r['ratio']:.3f}  tail {r['tail']:.3f}  share exact {r['exact']:.5f} core {r['core']:.5f}"
             + (f" offset {r['offset']:.5f}" if "offset" in r else "") + f"  oracle bits {r['oracle']}" for (s, fn), r in sorted(REPORT.items())]
    print("\nlargest |got - f64| / bound per site, mismatch shares, outputs differing from the oracle's fp32 formula:\n" + "\n".join(lines))
    off = {k: r["ratio"] for k, r in REPORT.items() if not 0.05 < r["ratio"] <= 1.0}
    assert not off, f"ratio outside (0.05, 1] on {off}"
