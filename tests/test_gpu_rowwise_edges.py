"""GPU: every kernel of csrc/hv_rowwise.hip at its dispatch and loop edges, against the fp64 references and per-element bounds of
tests/rowwise_bounds.py (what those bounds accept and reject: tests/test_rowwise_bounds_cpu.py).

Every operand sits in NaN-poisoned memory (rows before and after, columns [D, ld)), every output in a sentinel-filled buffer whose
cells outside the view keep their bits, and a second launch gives the same bits.  The largest error-to-bound ratio of each kernel is
printed at the end (test_zz_ratio_report) and must be above 0.05 - a bound that loose would catch nothing.

  ln_modulate (bf16, fp8)   D on both sides of every MAXC boundary (512|520, 2048|2056, 3072|3080), a ragged last chunk group (1000),
                            D = 8, M in {1, 4, 5, 9}, padded ldx / ldo, the five shift / scale / affine modes, four data classes
  quant_rows_fp8            a second trip of the lane loop (K = 520), M % 4 != 0, strided rows, the row-scale floor 2^-126
  qknorm_rope (+ scatter)   2H = 16 (one trip of the head loop) and 18 (a ragged second trip), a poisoned gap between q and k, tables
                            with an independent value per column, poisoned from row n_rope on; every heads_per_block
  linear_smallm             every M, K across the 512-element lane stride, N % 4 != 0, padded ldx / ldo, all flag combinations
  timestep_embedding, euler_step (the scalar tail), patchify / unpatchify, masked_mean / broadcast_row, fp8_dequant and copy3d (the
  second grid-stride trip)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402
from tests import error_bounds as EB  # noqa: E402
from tests import rowwise_bounds as RB  # noqa: E402
from tests.guarded_memory import NAN_BITS, Guarded, GuardedBytes, GuardedFlat, Poisoned, bits, poisoned_vec, same_bits  # noqa: E402

DEV = "cuda"
BF16, F16, F32, FP8 = torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn
RATIOS = {}


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.load()
    return _ops


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 47, DEV) * (scale * math.sqrt(3.0))


def _record(kernel, r):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)


def within_ulp(got, ref, dtype):
    g, r = got.double(), ref.double()
    tol = torch.maximum(EB.ulp_out(g, dtype), EB.ulp_out(r, dtype))
    return float(((g - r).abs() / tol).max())


# ---------------------------------------------------------------------------------------------------- ln_modulate (bf16 and fp8)
LN_MODES = ["shift+scale", "scale", "shift", "neither", "affine"]


def _ln_operands(D, mode, key):
    shift = poisoned_vec(U((D,), key + ".shift", 0.5).to(BF16)) if mode in ("shift+scale", "shift", "affine") else None
    if mode == "affine":
        mul = poisoned_vec((1.0 + U((D,), key + ".w", 0.3)).to(BF16))
    else:
        mul = poisoned_vec(U((D,), key + ".scale", 0.5).to(BF16)) if mode in ("shift+scale", "scale") else None
    return shift, mul


def _ln_case(ops, M, D, mode, cls, shares):
    what = f"ln_modulate M={M} D={D} {mode} {cls}"
    x = RB.data_rows(cls, M, D, f"ln.{D}").to(DEV)
    X = Poisoned(x, 3, 5, 24)
    shift, mul = _ln_operands(D, mode, f"ln.{D}.{mode}")
    o = Guarded(M, D, BF16, pad=16)
    ops.ln_modulate(X.view, shift, mul, out=o.view, affine=mode == "affine")
    assert o.intact() and X.intact(), f"{what}: a store outside the output"
    y = o.view.clone()
    y64, bound = RB.ln_ref(x, shift, mul, affine=mode == "affine")
    _record("ln_modulate_bf16", RB.check(y, y64, bound, what))
    shares.append((int((y != y64.to(BF16)).sum()), y.numel(), cls))
    if cls == "constant":                            # (x - mean) is exactly zero and eps keeps rstd finite: the output is the shift
        want = torch.zeros(M, D, dtype=BF16, device=DEV) if shift is None else shift.expand(M, D)
        assert torch.equal(y, want), f"{what}: a constant row must give the shift"
    ops.ln_modulate(X.view, shift, mul, out=o.view, affine=mode == "affine")
    assert same_bits(o.view, y), f"{what}: a second launch differs"
    if mode == "affine":
        return
    # the fp8 form: the same bf16 values, then the row quantisation of oracle.dit_ref.fp8_quant_rows, bit for bit
    ldq = (D + 15) // 16 * 16 + 16
    q, s = GuardedBytes(M, D, ldq), GuardedFlat(M, F32)
    ops.ln_modulate_fp8(X.view, shift, mul, out_q=q.view, out_scale=s.view)
    assert q.intact() and s.intact() and X.intact(), f"{what} fp8: a store outside the codes or scales"
    q_ref, s_ref = R.fp8_quant_rows(y.cpu())
    assert same_bits(s.view.cpu(), s_ref.reshape(-1)), f"{what} fp8: row scales differ from amax(bf16 output) * (1/448)"
    assert same_bits(q.view.cpu(), q_ref.to(FP8)), f"{what} fp8: codes differ from the oracle's quantisation of the bf16 output"
    assert bool(torch.isfinite(q.view.float()).all()) and bool(torch.isfinite(s.view).all())


def _ln_shares_ok(shares, what):
    for cls in set(c for _, _, c in shares):
        bad = sum(b for b, _, c in shares if c == cls)
        n = sum(k for _, k, c in shares if c == cls)
        share = bad / n
        print(f"{what} {cls}: {bad} of {n} outputs differ in bits from bf16(fp64 reference): share {share:.4f}, cap {RB.mismatch_cap('ln.' + cls, n):.4f}")
        assert share <= RB.mismatch_cap("ln." + cls, n), f"{what} {cls}: mismatch share {share:.4f} above the cap - a contract rounding is skipped"


@pytest.mark.parametrize("D", RB.LN_DS)
def test_ln_modulate_every_mode_and_class(ops, D):
    shares = []
    for mode in LN_MODES:
        for cls in RB.LN_CLASSES:
            _ln_case(ops, 5, D, mode, cls, shares)
    _ln_shares_ok(shares, f"ln_modulate D={D}")


@pytest.mark.parametrize("M", [1, 4, 9])
def test_ln_modulate_row_counts(ops, M):
    shares = []
    for D in (8, 520, 1000, 3080, 4096):
        _ln_case(ops, M, D, "shift+scale", "control", shares)
        _ln_case(ops, M, D, "affine", "massive", shares)
    _ln_shares_ok(shares, f"ln_modulate M={M}")


# ---------------------------------------------------------------------------------------------------- quant_rows_fp8
def _quant_case(ops, x, what):
    M, K = x.shape
    X = Poisoned(x, 3, 5, 8)
    ldq = (K + 15) // 16 * 16 + 16                  # K + 16 rounded up: the kernel wants a 16-byte row stride
    q, s = GuardedBytes(M, K, ldq), GuardedFlat(M, F32)
    ops.quant_rows_fp8(X.view, out_q=q.view, out_scale=s.view)
    assert q.intact() and s.intact() and X.intact(), f"{what}: a store outside the codes or scales"
    q_ref, s_ref = R.fp8_quant_rows(x.cpu())
    assert bool(torch.isfinite(q.view.float()).all()) and bool(torch.isfinite(s.view).all()), f"{what}: not finite"
    assert same_bits(s.view.cpu(), s_ref.reshape(-1)), f"{what}: row scales {s.view.tolist()[:5]} differ from the oracle's {s_ref.reshape(-1).tolist()[:5]}"
    assert same_bits(q.view.cpu(), q_ref.to(FP8)), f"{what}: codes differ from the oracle's"
    q0 = q.view.clone()
    ops.quant_rows_fp8(X.view, out_q=q.view, out_scale=s.view)
    assert same_bits(q.view, q0), f"{what}: a second launch differs"
    return q_ref, s_ref


@pytest.mark.parametrize("K", [8, 512, 520, 3072])
@pytest.mark.parametrize("M", [1, 5])
def test_quant_rows_fp8(ops, M, K):
    for cls in ("control", "massive"):
        _quant_case(ops, RB.data_rows(cls, M, K, f"quant.{K}").to(DEV), f"quant_rows_fp8 {M}x{K} {cls}")


@pytest.mark.parametrize("K", [8, 520])
def test_quant_rows_fp8_special_rows(ops, K):
    """all zero (scale 1, codes 0); the maximum alone in the last column; a maximum equal to the largest finite bf16; amax = 2^-125 and
    2^-130 with zeros elsewhere: amax / 448 is below the smallest normal fp32 there, the row scale is floored at 2^-126 and every code
    is finite (without the floor 1 / s = inf and the zeros of the row became NaN)"""
    x = torch.zeros(5, K, dtype=BF16, device=DEV)
    x[1] = (U((K,), "quant.sp", 0.1)).to(BF16)
    x[1, K - 1] = 7.0
    x[2] = (U((K,), "quant.sp2", 1e30)).to(BF16)
    x[2, 3] = -torch.finfo(BF16).max
    x[3, 3] = 2.0 ** -125
    x[4, K - 2] = -(2.0 ** -130)
    q, s = _quant_case(ops, x, f"quant_rows_fp8 special rows K={K}")
    assert float(s[0]) == 1.0 and not bool(q[0].any())
    assert float(q[1, K - 1]) == 448.0 and float(q[2, 3]) == -448.0
    assert float(s[3]) == 2.0 ** -126 and float(s[4]) == 2.0 ** -126
    assert float(q[3, 3]) == 2.0 and float(q[4, K - 2]) == -0.0625 and int((q[3:] != 0).sum()) == 2


# ---------------------------------------------------------------------------------------------------- qknorm_rope (+ scatter)
def _qk_buffers(row, H):
    """the fused rows [5, ld = 3 H 128 + 64] in poisoned memory: q | a NaN gap of 128 | k | what is left of v"""
    k_off = H * 128 + 128
    W = 3 * H * 128 + 40
    t = row[:, :W].clone().to(DEV)
    t[:, H * 128:k_off] = float("nan")
    return Poisoned(t, 3, 5, 24), t, k_off


def _heads(view, H, k_off):
    return torch.cat([view[:, :H * 128], view[:, k_off:k_off + H * 128]], 1).reshape(view.shape[0], 2 * H, 128)


def _tables(n_rows, n_rope, key):
    if n_rope == 0:
        return None, None, None, None
    cos, sin = RB.rope_tables_independent(n_rows, key)
    cp, sp = cos.clone().to(DEV), sin.clone().to(DEV)
    cp[n_rope:], sp[n_rope:] = float("nan"), float("nan")
    return cos.to(DEV), sin.to(DEV), cp, sp


@pytest.mark.parametrize("cls", RB.QK_CLASSES)
@pytest.mark.parametrize("H", RB.QK_HEADS)
def test_qknorm_rope_in_place(ops, H, cls):
    for n_rows, n_rope in RB.QK_ROWS:
        what = f"qknorm_rope H={H} rows={n_rows} n_rope={n_rope} {cls}"
        key = f"qk.{H}.{n_rope}"
        row, x, w, qw, kw = RB.qk_case(cls, H, n_rows, key)
        cos, sin, cp, sp = _tables(n_rows, n_rope, key)
        Q, t0, k_off = _qk_buffers(row, H)
        assert Q.view.stride(0) == 3 * H * 128 + 64
        qwp, kwp = poisoned_vec(qw.to(DEV)), poisoned_vec(kw.to(DEV))
        ops.qknorm_rope_(Q.view, qwp, kwp, cp, sp, n_rope, H, k_off)
        assert Q.intact(), f"{what}: a store outside the rows"
        got = _heads(Q.view, H, k_off).clone()
        rest = torch.ones_like(t0, dtype=torch.bool)
        rest[:, :H * 128] = False
        rest[:, k_off:k_off + H * 128] = False
        assert torch.equal(bits(Q.view)[rest], bits(t0)[rest]), f"{what}: the gap between q and k or v changed"
        y64, bound, amb, amb_bound = RB.qknorm_ref(x.to(DEV), w.to(DEV), cos, sin, n_rope)
        assert bool(torch.isfinite(got.float()).all()), f"{what}: not finite"
        _record("qknorm_rope_bf16", RB.check(got.reshape(-1, 128), y64.reshape(-1, 128), bound.reshape(-1, 128), what, skip=amb.reshape(-1, 128)))
        assert bool(((got.double() - y64).abs() <= amb_bound)[amb].all()), f"{what}: an ambiguous element is more than 2 ulp off"
        share = RB.mismatch_share(got, y64, BF16, amb)
        assert share <= RB.mismatch_cap("qknorm", got.numel()), f"{what}: mismatch share {share:.5f}: a contract rounding is skipped or doubled"
        Q2, _, _ = _qk_buffers(row, H)
        ops.qknorm_rope_(Q2.view, qwp, kwp, cp, sp, n_rope, H, k_off)
        assert same_bits(Q2.view, Q.view), f"{what}: a second launch differs"


@pytest.mark.parametrize("H", RB.QK_HEADS)
def test_qknorm_rope_scatter(ops, H):
    for n_rows, n_rope in RB.QK_ROWS:                      # n_rope = 0: NULL tables through the scatter form's own argument checks
        _scatter_case(ops, H, n_rows, n_rope, "control")
    _scatter_case(ops, H, 5, 4, "massive")


def _scatter_case(ops, H, n_rows, n_rope, cls):
    key = f"qk.{H}.{n_rope}"
    row, x, w, qw, kw = RB.qk_case(cls, H, n_rows, key)
    cos, sin, cp, sp = _tables(n_rows, n_rope, key)
    qwp, kwp = poisoned_vec(qw.to(DEV)), poisoned_vec(kw.to(DEV))
    Q, t0, k_off = _qk_buffers(row, H)
    ops.qknorm_rope_(Q.view, qwp, kwp, cp, sp, n_rope, H, k_off)
    want = _heads(Q.view, H, k_off).clone()
    for hpb in sorted({h for h in (1, 2, 3) if (2 * H) % h == 0} | {2 * H}):
        what = f"qknorm_rope_scatter H={H} heads_per_block={hpb}"
        S, s0, _ = _qk_buffers(row, H)
        nblk = 2 * H // hpb
        buf = torch.full((nblk, n_rows + 3, hpb * 128 + 64), 0x7E5A, dtype=torch.int16, device=DEV)
        dst = buf.view(BF16)[:, 1:1 + n_rows, :hpb * 128].permute(1, 0, 2)          # [rows, blocks, hpb * 128], dst_ld = hpb * 128 + 64
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[:, 1:1 + n_rows, :hpb * 128] = False
        ops.qknorm_rope_(S.view, qwp, kwp, cp, sp, n_rope, H, k_off, out=dst)
        assert bool((buf[mask] == 0x7E5A).all()), f"{what}: a store outside the destination"
        assert S.intact() and same_bits(S.view, s0), f"{what}: the source rows changed"
        assert same_bits(dst.reshape(n_rows, 2 * H, 128), want), f"{what}: differs from the in-place result"


# ---------------------------------------------------------------------------------------------------- linear_smallm
@pytest.mark.parametrize("K", [8, 256, 512, 520, 3080])
def test_linear_smallm(ops, K):
    silu = lambda v: RB.silu64(v).to(BF16)
    bad_in = n_in = 0
    for M in (1, 2, 3, 4):
        for N in (1, 3, 5, 41):
            for with_bias in (True, False):
                what = f"linear_smallm {M}x{N}x{K} bias={with_bias}"
                x, w, b = (t.to(DEV) for t in RB.gemv_operands(M, N, K, f"gemv.{M}.{N}.{K}"))
                X = Poisoned(x, 3, 5, 8)
                Wp = poisoned_vec(w.reshape(-1)).view(N, K)
                bp = poisoned_vec(b) if with_bias else None
                bb = b if with_bias else None

                def run(xin=X.view, **kw):
                    o = Guarded(M, N, BF16, pad=3)
                    ops.linear_smallm(xin, Wp, bp, out=o.view, **kw)
                    assert o.intact(), f"{what} {kw}: a store outside the output"
                    return o.view.clone()

                y = run()
                _record("linear_smallm_bf16", EB.check(y, EB.gemm_ref(x, w, bb), BF16, what))
                assert same_bits(run(), y), f"{what}: a second launch differs"
                r = within_ulp(run(silu_out=True), silu(y), BF16)
                assert r <= 1.0, f"{what}: silu_out {r:.2f} ulp from bf16(silu(y))"
                add = U((M, N), what + ".add").to(BF16)
                A = Poisoned(add, 2, 3, 3)                                     # the geometry of the output buffer
                o = Guarded(M, N, BF16, pad=3)
                ops.linear_smallm(X.view, Wp, bp, out=o.view, addend=A.view)
                assert o.intact() and A.intact()
                assert same_bits(o.view, (y.float() + add.float()).to(BF16)), f"{what}: addend"
                # silu_in on inputs whose silu is not near a bf16 tie: the operand bf16(silu(x)) is known exactly
                xs = RB.tie_free_for_silu(x)
                Xs = Poisoned(xs, 3, 5, 8)
                ref = EB.gemm_ref(silu(xs), w, bb)
                ys = run(Xs.view, silu_in=True)
                _record("linear_smallm_bf16", EB.check(ys, ref, BF16, what + " silu_in"))
                bad_in += int((ys != ref.y.to(BF16)).sum())
                n_in += ys.numel()
                r = within_ulp(run(Xs.view, silu_in=True, silu_out=True), silu(ys), BF16)
                assert r <= 1.0, f"{what}: silu_in + silu_out {r:.2f} ulp from bf16(silu(y))"
                assert X.intact() and Xs.intact()
    share = bad_in / n_in
    print(f"linear_smallm K={K} silu_in: {bad_in} of {n_in} outputs differ in bits from bf16(fp64 reference)")
    assert share <= RB.mismatch_cap("silu_in", n_in), f"K={K}: silu_in mismatch share {share:.4f}: SiLU(x) is not rounded to bf16"


# ---------------------------------------------------------------------------------------------------- timestep_embedding
@pytest.mark.parametrize("dim", [2, 256, 258])
def test_timestep_embedding(ops, dim):
    from hunyuanvideo_efficiency_amd import _lib
    batches = [[t] for t in RB.TS] + [RB.TS, [RB.TS[i % 7] + 0.25 * (i // 7) for i in range(129)]]
    for tl in batches:
        t = poisoned_vec(torch.tensor(tl, dtype=F32, device=DEV))
        n = len(tl)
        o = GuardedFlat(n * dim, BF16)
        _lib.call("timestep_embedding_bf16", t, o.view, n, dim, 10000.0)
        assert o.intact(), "timestep_embedding: a store outside the output"
        got = o.view.reshape(n, dim).clone()
        y64, bound = RB.timestep_ref(t, dim)
        _record("timestep_embedding_bf16", RB.check(got, y64, bound, f"timestep_embedding n_t={n} dim={dim}"))
        orc = R.timestep_embedding(t.cpu(), dim).to(BF16)
        print(f"timestep_embedding n_t={n} dim={dim}: {int((got.cpu() != orc).sum())} of {got.numel()} elements differ in bits from the fp32 oracle")
        assert same_bits(ops.timestep_embedding(t, dim), got)


# ---------------------------------------------------------------------------------------------------- euler_step
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025, 1027])
def test_euler_step(ops, n):
    dt = -0.0371
    s0 = U((n,), f"euler.s.{n}", 2.0)
    for name, v in (("euler_step_f32", U((n,), f"euler.v.{n}").to(BF16)), ("euler_step_f32_f32", U((n,), f"euler.v32.{n}"))):
        vp = poisoned_vec(v)
        g = GuardedFlat(n, F32)
        g.view.copy_(s0)
        (ops.euler_step_ if v.dtype == BF16 else ops.euler_step_f32_)(g.view, vp, dt)
        assert g.intact(), f"{name} n={n}: a store outside the sample"
        y64, bound = RB.euler_ref(s0, v, dt)
        _record(name, RB.check(g.view[None], y64[None], bound[None], f"{name} n={n}"))
        g2 = GuardedFlat(n, F32)
        g2.view.copy_(s0)
        (ops.euler_step_ if v.dtype == BF16 else ops.euler_step_f32_)(g2.view, vp, dt)
        assert same_bits(g2.view, g.view)


# ---------------------------------------------------------------------------------------------------- patchify / unpatchify
@pytest.mark.parametrize("C,T,H,W", [(16, 1, 2, 2), (16, 3, 6, 10), (4, 2, 4, 6)])
def test_patchify_unpatchify(ops, C, T, H, W):
    x = poisoned_vec(U((C * T * H * W,), f"patch.{C}.{T}.{H}.{W}")).view(C, T, H, W)
    ntok = T * (H // 2) * (W // 2)
    o = GuardedFlat(ntok * C * 4, BF16)
    ops.patchify(x, out=o.view.view(ntok, C * 4))
    assert o.intact()
    want = x.reshape(C, T, H // 2, 2, W // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(ntok, C * 4).to(BF16)
    assert same_bits(o.view.view(ntok, C * 4), want), "patchify"
    y = U((ntok, C * 4), f"unpatch.{C}.{T}.{H}.{W}").to(BF16)
    Y = Poisoned(y, 3, 5, 8)                                                   # ldy = 4 C + 8
    u = GuardedFlat(C * T * H * W, BF16)
    ops.unpatchify(Y.view, C, T, H, W, out=u.view.view(C, T, H, W))
    assert u.intact() and Y.intact()
    want = y.reshape(T, H // 2, W // 2, C, 2, 2).permute(3, 0, 1, 4, 2, 5).reshape(C, T, H, W)
    assert same_bits(u.view.view(C, T, H, W), want), "unpatchify"


# ---------------------------------------------------------------------------------------------------- masked_mean / broadcast_row
@pytest.mark.parametrize("L", [1, 32, 300])
@pytest.mark.parametrize("D", [1, 255, 256, 257, 520])
def test_masked_mean(ops, L, D):
    from hunyuanvideo_efficiency_amd import _lib
    masks = {"none": None, "ones": torch.ones(L, dtype=torch.int32), "last": torch.zeros(L, dtype=torch.int32),
             "prefix": (torch.arange(L) < max(1, (2 * L) // 5)).int()}
    masks["last"][L - 1] = 1
    for name, mask in masks.items():
        x = U((L, D), f"mm.{L}.{D}").to(BF16)
        if mask is not None:
            x[mask.to(DEV) == 0] = 1e30 * (1 if name == "last" else -1)          # must be multiplied away exactly
        xp = poisoned_vec(x.reshape(-1)).view(L, D)
        mp = None if mask is None else poisoned_vec(mask.to(DEV))
        o = GuardedFlat(D, BF16)                              # threads D .. 255 of the last block must not store
        _lib.call("masked_mean_bf16", xp, mp, o.view, L, D)
        assert o.intact(), f"masked_mean L={L} D={D} mask={name}: a store outside the output"
        got = o.view.clone()
        ref = RB.masked_mean_ref(x, None if mask is None else mask.to(DEV))
        _record("masked_mean_bf16", EB.check(got[None], ref, BF16, f"masked_mean L={L} D={D} mask={name}"))
        assert same_bits(ops.masked_mean(xp, mp), got)


@pytest.mark.parametrize("D", [8, 250])
@pytest.mark.parametrize("rows", [1, 5])
def test_broadcast_row(ops, rows, D):
    src = poisoned_vec(U((D,), f"bc.{D}").to(BF16))
    o = Guarded(rows, D, BF16, pad=6)
    ops.broadcast_row_(src, o.view)
    assert o.intact() and same_bits(o.view, src.expand(rows, D))


# ---------------------------------------------------------------------------------------------------- fp8_dequant
def test_fp8_dequant_every_code(ops):
    codes = torch.arange(256, dtype=torch.uint8, device=DEV)
    for sc in (1.0, 0.0123, 2.0 ** -20, -3.0):
        w8 = poisoned_vec(codes).view(FP8)
        scale = poisoned_vec(torch.tensor([sc], dtype=BF16, device=DEV))
        o = GuardedFlat(256, BF16)
        ops.fp8_dequant(w8, scale, o.view)
        assert o.intact()
        want = w8.to(BF16) * scale
        nan = torch.isnan(want.float())
        assert int(nan.sum()) == 2 and torch.equal(torch.isnan(o.view.float()), nan), "the two NaN codes, and only they, give NaN"
        assert torch.equal(bits(o.view)[~nan], bits(want)[~nan]), f"fp8_dequant scale {sc}"


def test_fp8_dequant_second_grid_stride_trip(ops):
    n = 16384 * 256 * 8 + 8                       # one vector more than the capped grid covers in its first trip
    w8 = (torch.arange(n, dtype=torch.int32, device=DEV) * 37 % 251).to(torch.uint8)
    w8[(w8 & 0x7F) == 0x7F] = 0x11                # keep NaN codes out of the bitwise comparison
    w8 = w8.view(FP8)
    scale = torch.tensor([0.0123], dtype=BF16, device=DEV)
    o = GuardedFlat(n, BF16)
    ops.fp8_dequant(w8, scale, o.view)
    assert o.intact()
    assert torch.equal(o.view, w8.to(BF16) * scale)


# ---------------------------------------------------------------------------------------------------- copy3d
def _copy3d_case(ops, n_batch, rows, cols):
    src = U((n_batch, rows, cols), f"c3.{n_batch}.{rows}.{cols}").to(BF16)
    sld, dld = cols + 8, cols + 24
    sbs, dbs = (rows + 2) * sld, (rows + 1) * dld
    sbuf = torch.full((n_batch * sbs + 64,), NAN_BITS[2], dtype=torch.int16, device=DEV).view(BF16)
    sv = sbuf[16:16 + n_batch * sbs].view(n_batch, rows + 2, sld)[:, :rows, :cols]
    sv.copy_(src)
    dbuf = torch.full((n_batch * dbs + 64,), 0x7E5A, dtype=torch.int16, device=DEV)
    dv = dbuf.view(BF16)[24:24 + n_batch * dbs].view(n_batch, rows + 1, dld)[:, :rows, :cols]
    mask = torch.ones_like(dbuf, dtype=torch.bool)
    mask[24:24 + n_batch * dbs].view(n_batch, rows + 1, dld)[:, :rows, :cols] = False
    ops.copy3d(sv, dv, n_batch, rows, cols, sbs, sld, dbs, dld)
    assert bool((dbuf[mask] == 0x7E5A).all()), "copy3d: a store outside the destination"
    assert same_bits(dv, src), "copy3d"


@pytest.mark.parametrize("n_batch", [1, 3])
@pytest.mark.parametrize("cols", [8, 136])
@pytest.mark.parametrize("rows", [1, 7])
def test_copy3d(ops, rows, cols, n_batch):
    _copy3d_case(ops, n_batch, rows, cols)


def test_copy3d_second_grid_stride_trip(ops):
    _copy3d_case(ops, 1, 8193, 1024)              # rows * cols / 8 = 4096 * 256 + 128


# ---------------------------------------------------------------------------------------------------- the ratios
def test_zz_ratio_report():
    """largest error-to-bound ratio per kernel over this module's cases (run after them); below 0.05 the bound would be too loose
    there to catch anything"""
    print("\nlargest |got - y64| / bound per kernel:\n" + "\n".join(f"  {k:<26} {RATIOS[k]:.3f}" for k in sorted(RATIOS)))
    low = {k: r for k, r in RATIOS.items() if not 0.05 < r <= 1.0}
    assert not low, f"bound too loose on {low}"
