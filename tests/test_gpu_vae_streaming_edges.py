"""GPU: the streaming half of csrc/hv_vae.hip - groupnorm_apply, softmax_rows, transpose_16b, temporal_resample, blend, copy4d,
latent_tile, postprocess - at the edges of their thread maps and of the capped grids (grid_for: 8192 blocks, then a grid-stride loop),
against the fp64 references and bounds of tests/rowwise_bounds.py.  Operands in NaN-poisoned memory, outputs in sentinel-filled
buffers, a second launch gives the same bits; the largest error-to-bound ratio per kernel is printed by test_zz_ratio_report and must
be above 0.05.

  groupnorm_apply    C = 96 (12 chunk threads, 21 rows per step, four idle threads), 8 and 2048; M around 4 * nrl; padded strides
  softmax_rows       rows longer than one trip of the 1024 / 256 column loops; the vector and the scalar kernel; NaN behind `valid`
  temporal_resample, blend, copy4d, latent_tile, postprocess: one launch each above the grid cap (the second grid-stride trip)"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import vae_ref as VR  # noqa: E402
from tests import rowwise_bounds as RB  # noqa: E402
from tests.guarded_memory import NAN_BITS, Guarded, GuardedFlat, Poisoned, bits, crop, poisoned_vec, same_bits  # noqa: E402

DEV = "cuda"
F16, F32 = torch.float16, torch.float32
E = VR.Prec(True)
RATIOS = {}
TAIL = 8192 * 256 + 3                      # elements: one grid-stride trip of the capped grid and three more


@pytest.fixture(scope="module")
def V():
    from hunyuanvideo_efficiency_amd import vae_ops, _lib
    _lib.load()
    return vae_ops


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 53, DEV) * (scale * math.sqrt(3.0))


def _record(kernel, r):
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), r)


# ---------------------------------------------------------------------------------------------------- groupnorm_apply
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C", [8, 32, 96, 128, 2048])
def test_groupnorm_apply(V, C, silu):
    nrl = 256 // (C // 8)
    aff = poisoned_vec(torch.stack([1.0 + U((C,), f"gn.sc.{C}", 0.5), U((C,), f"gn.sh.{C}", 1.0)], 1).reshape(-1)).view(C, 2)
    for M in (1, nrl + 1, 4 * nrl - 1, 4 * nrl, 4 * nrl + 1, 9 * nrl + 2):
        what = f"groupnorm_apply M={M} C={C} silu={silu}"
        x = U((M, C), f"gn.x.{M}.{C}", 2.0).to(F16)
        X = Poisoned(x, 3, 5, 8)
        o = Guarded(M, C, F16, pad=16)
        V.groupnorm_apply(X.view, aff, silu, out=o.view)
        assert o.intact() and X.intact(), f"{what}: a store outside the output"
        y = o.view.clone()
        y64, bound = RB.gn_apply_ref(x, aff, silu)
        _record("groupnorm_apply_f16", RB.check(y, y64, bound, what))
        V.groupnorm_apply(X.view, aff, silu, out=o.view)
        assert same_bits(o.view, y), f"{what}: a second launch differs"


# ---------------------------------------------------------------------------------------------------- softmax_rows
def _softmax_case(V, cls, rows, cols, cols_pad, cb, scale, offset_view=False):
    what = f"softmax_rows {cls} {rows}x{cols} pad={cols_pad} causal_block={cb} offset_view={offset_view}"
    s = RB.softmax_scores(cls, rows, cols, f"sm.{cols}").to(DEV)
    valid = RB.valid_of(rows, cols, cb).to(DEV)
    sp = s.clone()
    sp[torch.arange(cols, device=DEV)[None] >= valid[:, None]] = float("nan")          # a NaN in any output is a mask failure
    if offset_view:                                                                      # a vector-eligible shape, one float off 16 bytes
        flat = torch.full((rows * (cols + 12) + 8,), float("nan"), dtype=F32, device=DEV)
        S_view = flat[1:1 + rows * (cols + 12)].view(rows, cols + 12)[:, :cols]
        S_view.copy_(sp)
    else:
        S = Poisoned(sp, 3, 5, 12)                                                       # ld_s = cols + 12
        S_view = S.view
    o = Guarded(rows, cols_pad, F16, pad=16)
    V.softmax_rows(S_view, cols, cols_pad, scale, out=o.view, causal_block=cb)
    assert o.intact(), f"{what}: a store outside the output"
    p = o.view.clone()
    assert bool(torch.isfinite(p.float()).all()), f"{what}: a masked column reached an output"
    p64, bound = RB.softmax_ref(s, valid, scale)
    _record("softmax_rows_f32_f16", RB.check(p[:, :cols], p64, bound, what))
    colp = torch.arange(cols_pad, device=DEV)[None]
    assert not bool(bits(p)[colp.expand(rows, cols_pad) >= valid[:, None]].any()), f"{what}: columns [valid, cols_pad) must be +0"
    dev = (p.float().sum(-1) - 1.0).abs()
    assert bool((dev <= valid.float() * 2.0 ** -12).all()), f"{what}: a row sum is {float(dev.max()):.2e} from 1"
    V.softmax_rows(S_view, cols, cols_pad, scale, out=o.view, causal_block=cb)
    assert same_bits(o.view, p), f"{what}: a second launch differs"


@pytest.mark.parametrize("cls", RB.SOFTMAX_CLASSES)
@pytest.mark.parametrize("cols", [4, 1020, 1024, 1028, 2052, 1, 70, 257, 1025])
def test_softmax_rows(V, cols, cls):
    for cols_pad in sorted({cols, (cols + 63) // 64 * 64}):
        for cb in (0, 4, 7, 1024):
            _softmax_case(V, cls, 9, cols, cols_pad, cb, 0.7)


def test_softmax_rows_misaligned_base_takes_the_scalar_kernel(V):
    _softmax_case(V, "flat", 9, 1028, 1088, 4, 0.7, offset_view=True)


# ---------------------------------------------------------------------------------------------------- transpose_16b
@pytest.mark.parametrize("R_,C_", [(1, 1), (1, 33), (31, 32), (32, 31), (33, 300), (300, 1), (32, 32), (300, 33), (31, 300)])
def test_transpose_16b(V, R_, C_):
    x = U((R_, C_), f"tr.{R_}.{C_}").to(F16)
    X = Poisoned(x, 3, 5, 7)
    o = Guarded(C_, R_, F16, pad=5)
    V.transpose_16b(X.view, o.view)
    assert o.intact() and X.intact() and same_bits(o.view, x.T)


# ---------------------------------------------------------------------------------------------------- temporal_resample
def _temporal_case(V, T_in, HW, C, k, s, mode):
    from hunyuanvideo_efficiency_amd import _lib
    what = f"temporal_resample T={T_in} HW={HW} C={C} k={k} s={s} mode={mode}"
    x = U((T_in * HW, C), f"tp.{T_in}.{HW}.{C}", 2.0).to(F16)
    X = Poisoned(x, 3, 5, 8)
    t_out = T_in * s if mode == 1 else (T_in - 1) // s + 1
    o = Guarded(t_out * HW, C, F16, pad=16)
    _lib.call("temporal_resample_f16", X.view, X.view.stride(0), o.view, o.view.stride(0), T_in, HW, C, mode, k, s)
    assert o.intact() and X.intact(), f"{what}: a store outside the output"
    if mode == 1:
        want = x.reshape(T_in, 1, HW, C).expand(T_in, s, HW, C).reshape(t_out * HW, C)
        assert same_bits(o.view, want), what
    else:
        y64, bound = RB.temporal_avg_ref(x, T_in, HW, k, s)
        r = RB.check(o.view, y64, bound, what)
        if k > 1:
            _record("temporal_resample_f16", r)


@pytest.mark.parametrize("T_in", [1, 2, 5])
@pytest.mark.parametrize("C", [8, 72])
def test_temporal_resample(V, T_in, C):
    for HW in (1, 7):
        for s in (1, 2, 3):
            _temporal_case(V, T_in, HW, C, 1, s, 1)
            for k in (1, 2, 3, 4):
                _temporal_case(V, T_in, HW, C, k, s, 0)


def test_temporal_resample_second_grid_stride_trip(V):
    _temporal_case(V, 5, 5500, 1024, 3, 2, 0)          # t_out * HW * C / 8 = 3 * 5500 * 128 > 8192 * 256


# ---------------------------------------------------------------------------------------------------- blend, copy4d, latent_tile, postprocess
def _blend_want(a, b, axis, extent):
    n = a.shape[axis]
    y = torch.arange(n, dtype=torch.float64, device=DEV)
    shape = [1, 1, 1, 1]
    shape[axis] = n
    wa, wb = (1.0 - y / extent).float().reshape(shape), (y / extent).float().reshape(shape)      # double division, one cast to fp32
    return ((a.float() * wa).half().float() + (b.float() * wb).half().float()).half()


def _blend_case(V, dims, axis, extent, ma=(1, 2, 1, 3), mb=(2, 1, 3, 1)):
    what = f"blend dims={dims} axis={axis} extent={extent}"
    a, b = U(dims, f"bl.a.{dims}.{axis}", 2.0).to(F16), U(dims, f"bl.b.{dims}.{axis}", 2.0).to(F16)
    abuf, av, amask = crop(dims, F16, what, margin=ma)
    bbuf, bv, bmask = crop(dims, F16, what, margin=mb, poison=False)
    av.copy_(a), bv.copy_(b)
    V.blend_(av, bv, axis, extent)
    assert bool((bbuf[bmask] == 0x7E5A).all()) and bool((abuf[amask] == NAN_BITS[2]).all()), f"{what}: a store outside the view"
    assert same_bits(av, a), f"{what}: the first operand changed"
    assert same_bits(bv, _blend_want(a, b, axis, extent)), what


@pytest.mark.parametrize("axis", [0, 1, 2, 3])
@pytest.mark.parametrize("extent", [1, 3, 8])
def test_blend(V, axis, extent):
    for n in sorted({1, extent}):
        dims = [3, 2, 5, 6]
        dims[axis] = n
        _blend_case(V, tuple(dims), axis, extent)


def test_blend_second_grid_stride_trip(V):
    _blend_case(V, (1, 1, 8, TAIL // 8 + 1), 2, 8, ma=(0, 0, 1, 8), mb=(0, 0, 0, 3))


def test_copy4d_permuted_strides(V):
    dims = (3, 4, 5, 6)
    src = U(dims, "c4").to(F16)
    sbuf, sv, _ = crop((6, 5, 4, 3), F16, "c4s")
    sv = sv.permute(3, 2, 1, 0)                         # [3,4,5,6] with reversed strides
    sv.copy_(src)
    dbuf, dv, dmask = crop((4, 3, 6, 5), F16, "c4d", poison=False)
    dv = dv.permute(1, 0, 3, 2)
    V.copy4d_(sv, dv)
    assert bool((dbuf[dmask] == 0x7E5A).all()) and same_bits(dv, src)


def test_copy4d_second_grid_stride_trip(V):
    dims = (1, 1, 1, TAIL)
    src = U(dims, "c4t").to(F16)
    dbuf, dv, dmask = crop(dims, F16, "c4td", margin=(0, 0, 0, 8), poison=False)
    V.copy4d_(src, dv)
    assert bool((dbuf[dmask] == 0x7E5A).all()) and same_bits(dv, src)


def _latent_tile(z, cpad):
    """hv_vae_latent_tile_f16 into a guarded output"""
    from hunyuanvideo_efficiency_amd import _lib
    c, t, h, w = z.shape
    o = GuardedFlat(t * h * w * cpad, F16)
    _lib.call("vae_latent_tile_f16", z, *z.stride(), c, t, h, w, cpad, o.view)
    assert o.intact(), "latent_tile: a store outside the output"
    return o.view.view(t * h * w, cpad)


def _postprocess(x):
    """hv_vae_postprocess_f16_f32 into a guarded output"""
    from hunyuanvideo_efficiency_amd import _lib
    o = GuardedFlat(x.numel(), F32)
    _lib.call("vae_postprocess_f16_f32", x, o.view, x.numel())
    assert o.intact(), "postprocess: a store outside the output"
    return o.view


@pytest.mark.parametrize("cpad", [16, 64])
def test_latent_tile(V, cpad):
    dims = (16, 3, 5, 6)
    zbuf, zv, _ = crop(dims, F32, "lt")
    z = U(dims, "lt.z", 3.0)
    zv.copy_(z)
    want = torch.zeros(3 * 5 * 6, cpad, dtype=F16, device=DEV)
    want[:, :16] = z.permute(1, 2, 3, 0).reshape(-1, 16).half()
    assert same_bits(_latent_tile(zv, cpad), want) and same_bits(V.latent_tile(zv, cpad), want)
    zw, ww = zv[..., ::2], want.reshape(3, 5, 6, cpad)[:, :, ::2].reshape(-1, cpad)      # a view with sw = 2
    assert zw.stride(3) == 2 and same_bits(_latent_tile(zw, cpad), ww)


def test_latent_tile_second_grid_stride_trip(V):
    W = TAIL // 16 + 1
    z = U((16, 1, 1, W), "lt.tail")
    assert same_bits(_latent_tile(z, 16), z.permute(1, 2, 3, 0).reshape(-1, 16).half())


def test_postprocess_every_fp16_value(V):
    """all 65,536 fp16 bit patterns in one launch, bit for bit against the oracle; a NaN stays a NaN, as torch's clamp keeps it"""
    x = poisoned_vec(torch.arange(65536, dtype=torch.int32, device=DEV).to(torch.int16).view(F16))
    got = _postprocess(x).cpu()
    want = VR.postprocess(x.float().cpu(), E)
    nan = torch.isnan(want)
    assert int(nan.sum()) == 2046 and torch.equal(torch.isnan(got), nan), "a NaN input must give a NaN"
    assert torch.equal(bits(got)[~nan], bits(want)[~nan]), "postprocess differs from the oracle"
    assert torch.equal(torch.isnan(V.postprocess(x)).cpu(), nan)


def test_postprocess_second_grid_stride_trip(V):
    x = U((TAIL,), "pp.tail", 1.0).to(F16)
    assert same_bits(_postprocess(x), (x / 2 + 0.5).clamp(0, 1).float())


# ---------------------------------------------------------------------------------------------------- the ratios
def test_zz_ratio_report():
    """largest error-to-bound ratio per kernel over this module's cases (run after them); below 0.05 the bound would be too loose
    there to catch anything"""
    print("\nlargest |got - y64| / bound per kernel:\n" + "\n".join(f"  {k:<26} {RATIOS[k]:.3f}" for k in sorted(RATIOS)))
    low = {k: r for k, r in RATIOS.items() if not 0.05 < r <= 1.0}
    assert not low, f"bound too loose on {low}"
