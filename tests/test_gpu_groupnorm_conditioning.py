"""GroupNorm statistics on ill-conditioned activations: group means far from zero relative to the group's std (R = |mean| / std
of 10 .. 1000), near-constant and exactly constant groups, values at the fp16 limit.  One-pass moments in fp32 (var = E[x^2] -
mean^2) lose the variance there (relative error ~2^-24 R^2 per partial); the reference's nn.GroupNorm does not.  Every producer of
the statistics - the standalone pass (hv_groupnorm_affine_f16), the conv epilogues (hv_conv3d_causal_f16 and the sub-pixel
upsampler with `gn_partial`, folded by hv_groupnorm_finalize_f16) and the decoder tail that applies an affine in registers
(hv_conv3d_cout4_f16) - is checked against the definition, computed in fp64 with two passes on the STORED fp16 tensor:

    y_ref = (x - mean_g) * rstd_g * w + b

* affine check: y_k = x*sc + sh rebuilt in fp64 from the kernel's affine, |y_k - y_ref| <= 2e-4 (1 + |y_ref|).  (The shift alone is
  not compared: its error is multiplied by R and cancels against x*sc.)
* output check: hv_groupnorm_apply_f16, with and without SiLU, within 2 fp16 ulp of fp16(y_ref), the ulp taken at
  max(|y_ref|, 1/8): an fp32 affine cannot resolve y near zero better than its own representation error, |x sc| 2^-24 (up to
  ~1e-4 at R = 1000, one ulp at 1/8 is 1.2e-4).

The affine bound leaves room for that representation error up to R ~ 2000, so no class goes beyond (the near-constant conv data
sits at R ~ 1000).

The DiT norms (LayerNorm + modulate, its FP8 form, RMS q/k norm) are pinned on massive-activation, offset and constant rows too."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import vae_ref as R  # noqa: E402

DEV = "cuda:0"
F16 = torch.float16
E = R.Prec(True)
GROUPS, EPS = 32, 1e-6


@pytest.fixture(scope="module")
def V():
    from hunyuanvideo_efficiency_amd import vae_ops, _lib
    _lib.load()
    return vae_ops


def U(shape, key, device=DEV):
    """deterministic uniform in [-1, 1) (std 1/sqrt(3))"""
    return syn.hashed_uniform(shape, key, 5, device=device)


def group_sign(C):
    """per-channel sign of its group's offset: groups 0, 1 positive, 2, 3 negative, repeating"""
    g = torch.arange(C, device=DEV) // (C // GROUPS)
    return torch.where((g % 4) < 2, 1.0, -1.0)


def channel_spread(C):
    """0 in even groups (all channels of the group share one offset), j / cpg - 0.5 for channel j of an odd group"""
    cpg = C // GROUPS
    c = torch.arange(C, device=DEV)
    return torch.where((c // cpg) % 2 == 1, (c % cpg).float() / cpg - 0.5, 0.0)


# data classes: (mean, std) of every group, with the sign and spread above
CLASSES = {
    "control": None,                                # today's data: 0.3 + U * 2 sqrt(3)
    "offset10": (10.0, 1.0), "offset100": (100.0, 1.0), "offset300": (300.0, 1.0), "offset1000": (1000.0, 1.0),
    "nearconst1": (1.0, 3e-3), "nearconst8": (8.0, 0.05),
    "constant": "constant",                         # every value 0.3 (fp16 0.2998...): variance 0
    "fp16max": "fp16max",                           # +-(6e4 +- 4e3)
}


def make_x(kind, M, C, key):
    u = U((M, C), key)
    spec = CLASSES[kind]
    if spec is None:
        x = 0.3 + u * (2.0 * math.sqrt(3.0))
    elif spec == "constant":
        x = torch.full((M, C), 0.3, device=DEV)
    elif spec == "fp16max":
        x = group_sign(C) * (6e4 + 4e3 * u)
    else:
        mean, std = spec
        # odd groups: channel offsets spread over one std (the group std grows by ~30 %, R stays of the same order)
        x = group_sign(C) * (mean + std * channel_spread(C)) + u * (std * math.sqrt(3.0))
    return x.to(F16)


def ref_stats(x, C, chunk=1 << 22, groups=GROUPS, eps=EPS):
    """fp64 two-pass mean and rstd per group of fp16 rows x [M, C] (chunked over rows: the production size is 545 M values)"""
    M, cpg = x.shape[0], C // groups
    s = torch.zeros(groups, dtype=torch.float64, device=x.device)
    for r in range(0, M, chunk):
        s += x[r:r + chunk].double().reshape(-1, groups, cpg).sum((0, 2))
    mean = s / (M * cpg)
    q = torch.zeros_like(s)
    for r in range(0, M, chunk):
        q += ((x[r:r + chunk].double().reshape(-1, groups, cpg) - mean[None, :, None]) ** 2).sum((0, 2))
    var = q / (M * cpg)
    return mean, 1.0 / torch.sqrt(var + eps), var


AFFINE_TOL = 2e-4       # |x sc + sh - GroupNorm64(x)| <= 2e-4 (1 + |GroupNorm64(x)|): every affine path (own pass, conv epilogue, sub-pixel)


def affine_error(x, aff, w, b, rows=None, groups=GROUPS, eps=EPS):
    """(largest |x sc + sh - y_ref| / (1 + |y_ref|) over `rows` (default: all), y_ref) with y_ref the fp64 GroupNorm of x [M, C] at those
    rows; shared with tests/vae_wiring.py"""
    C = x.shape[1]
    cpg = C // groups
    mean, rstd, _ = ref_stats(x, C, groups=groups, eps=eps)
    mean_c, rstd_c = mean.repeat_interleave(cpg), rstd.repeat_interleave(cpg)
    xs = (x if rows is None else x[rows]).double()
    y_ref = (xs - mean_c) * rstd_c * w.double() + b.double()
    y_k = xs * aff[:, 0].double() + aff[:, 1].double()
    return ((y_k - y_ref).abs() / (1.0 + y_ref.abs())).max(), y_ref


def sample_rows(M, limit=1 << 18):
    """every row, or a deterministic spread of `limit` rows (first and last included) at large M"""
    if M <= limit:
        return torch.arange(M, device=DEV)
    return torch.unique(torch.cat([torch.linspace(0, M - 1, limit, device=DEV).long(), torch.tensor([M - 1], device=DEV)]))


def fp16_ulp(r16, floor=2.0 ** -3):
    """ulp of fp16 values, taken at max(|r|, floor)"""
    a = r16.double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=floor)))
    return torch.pow(2.0, e - 10)


def check(V, x, aff, w, b, silu_too=True, what=""):
    """affine check over every row (or a deterministic sample at large M) + output check of hv_groupnorm_apply_f16"""
    M, C = x.shape
    assert torch.isfinite(aff).all(), f"{what}: non-finite affine"
    rows = sample_rows(M)
    err, y_ref = affine_error(x, aff, w, b, rows)
    assert float(err) <= AFFINE_TOL, f"{what}: affine error {float(err):.3e} (bound 2e-4 (1 + |y|))"
    for silu in ((False, True) if silu_too else (False,)):
        got = V.groupnorm_apply(x, aff, silu)[rows]
        assert torch.isfinite(got).all(), f"{what}: non-finite output (silu={silu})"
        r = y_ref * torch.sigmoid(y_ref) if silu else y_ref
        r16 = r.to(F16)
        d = ((got.double() - r16.double()).abs() / fp16_ulp(r16)).max()
        assert float(d) <= 2.0, f"{what}: output {float(d):.2f} fp16 ulp from the fp64 reference (silu={silu})"
    return float(err)


def gn_params(C, key):
    return (1 + 0.1 * U((C,), key + ".w")).to(F16), (0.5 * U((C,), key + ".b")).to(F16)


# ---------------------------------------------------------------------------------------------------------------- standalone pass
@pytest.mark.parametrize("kind", list(CLASSES))
@pytest.mark.parametrize("M,C", [(105, 32), (1024, 128), (162, 512), (65536, 128), (4096, 32)])
def test_standalone_affine(V, kind, M, C):
    x = make_x(kind, M, C, f"sa.{M}.{C}.{kind}")
    w, b = gn_params(C, "sa")
    aff = V.groupnorm_affine(x, w, b, GROUPS, EPS)
    check(V, x, aff, w, b, what=f"standalone {kind} M={M} C={C}")
    if kind == "constant":          # true variance 0: rstd = 1/sqrt(eps), the output is b (to an fp16 ulp)
        got = V.groupnorm_apply(x, aff, False)
        d = (got.double() - b.double()).abs() / fp16_ulp(b)
        assert float(d.max()) <= 1.0, float(d.max())


# many rows per thread: 65 x 256 x 256 x 128 (1024 blocks x 16 row lanes x 260 rows) and 2^19 x 512 (4 row lanes x 256 rows)
@pytest.mark.parametrize("kind", ["offset300", "nearconst1", "control"])
@pytest.mark.parametrize("M,C", [(65 * 256 * 256, 128), (1 << 19, 512)])
def test_standalone_affine_many_rows_per_thread(V, kind, M, C):
    x = make_x(kind, M, C, f"sb.{kind}")
    w, b = gn_params(C, "sb")
    check(V, x, V.groupnorm_affine(x, w, b, GROUPS, EPS), w, b, what=f"standalone {kind} M={M} C={C}")


# ---------------------------------------------------------------------------------------------------------------- conv epilogues
def cl(x):
    """[1,C,T,H,W] -> channels-last rows [T*H*W, C] fp16"""
    return x[0].permute(1, 2, 3, 0).reshape(-1, x.shape[1]).contiguous().to(DEV).to(F16)


def taps(w):
    co, ci = w.shape[:2]
    return w.permute(0, 2, 3, 4, 1).reshape(co, 27, ci).to(DEV).to(F16).contiguous()


def offset_bias(C, level, key):
    """large biases, equal within each group (level +- 0.5, sign by group)"""
    g = torch.arange(C, device=DEV) // (C // GROUPS)
    return (group_sign(C) * (level + 0.5 * U((GROUPS,), key)[g])).to(F16)


# (bias level, weight scale): offset at R ~ 100 with std ~ 1, and near-constant groups (weights ~1e-3: std 0.02 - 0.05, R ~ 1000)
# (at 100 with weights 1e-3 the stored groups would be 1-3 fp16 levels, R ~ 3000: beyond what an fp32 shift can represent)
CONV_DATA = {"offset": (100.0, None), "nearconst": (30.0, 1e-3), "small_offset": (8.0, 1e-3), "control": (0.0, None)}


def conv_operands(T, H, W, Cin, Cout, data, key):
    level, wscale = CONV_DATA[data]
    x = U((1, Cin, T, H, W), key + ".x", device="cpu") * math.sqrt(3.0)
    wscale = wscale if wscale is not None else 1.0 / math.sqrt(27 * Cin) * math.sqrt(3.0)
    w = U((Cout, Cin, 3, 3, 3), key + ".w", device="cpu") * wscale
    b = offset_bias(Cout, level, key + ".b") if level else (0.1 * U((Cout,), key + ".b")).to(F16)
    return cl(x), taps(w), b


# every main loop that shares the epilogue (shapes of test_gpu_vae.py::test_conv_epilogue_groupnorm_statistics): 2-stage Cin 64,
# pipelined per-tap (W = 12), shift-reuse (W = 16), 256x256 (Cin = Cout = 256); ragged last tile; Cout 192 takes the strided fold
@pytest.mark.parametrize("data", list(CONV_DATA))
@pytest.mark.parametrize("T,H,W,Cin,Cout,with_res", [(3, 6, 5, 64, 64, False), (2, 7, 12, 128, 128, True), (3, 5, 16, 128, 64, False),
                                                     (2, 9, 16, 128, 128, True), (2, 6, 10, 256, 256, True), (1, 5, 7, 256, 512, False),
                                                     (2, 5, 9, 64, 192, False)])
def test_conv_epilogue_statistics(V, data, T, H, W, Cin, Cout, with_res):
    x, wt, b = conv_operands(T, H, W, Cin, Cout, data, f"ce.{Cin}.{Cout}")
    # residual variant: the offset rides on the residual (+-300, per group) instead of the bias
    res = make_x("offset300", T * H * W, Cout, "ce.res") if with_res else None
    out, st = V.conv3d_causal(x, wt, b, T, H, W, Cin, Cout, res=res, gn_stats=True)
    gw, gb = gn_params(Cout, "ce")
    check(V, out, V.groupnorm_affine_from_stats(st, gw, gb, GROUPS, EPS), gw, gb, what=f"epilogue {data} res={with_res}")


@pytest.mark.parametrize("data", ["offset", "nearconst"])
def test_conv_epilogue_statistics_two_level_fold(V, data):
    """65 x 256 x 256 x 128: 66,560 partial rows, folded in two levels"""
    T, H, W, C = 65, 256, 256, 128
    x, wt, b = conv_operands(T, H, W, C, C, data, "cf")
    out, st = V.conv3d_causal(x, wt, b, T, H, W, C, C, gn_stats=True)
    assert st.rows == 66560
    del x
    gw, gb = gn_params(C, "cf")
    check(V, out, V.groupnorm_affine_from_stats(st, gw, gb, GROUPS, EPS), gw, gb, what=f"two-level fold {data}")


@pytest.mark.parametrize("data", ["offset", "nearconst", "control"])
def test_subpixel_epilogue_statistics(V, data):
    T, H, W, C = 3, 5, 6, 256
    level, wscale = CONV_DATA[data]
    x = U((1, C, T, H, W), "sp.x", device="cpu") * math.sqrt(3.0)
    w = U((C, C, 3, 3, 3), "sp.w", device="cpu") * (wscale or math.sqrt(3.0 / (27 * C)))
    b = offset_bias(C, level, "sp.b") if level else (0.1 * U((C,), "sp.b")).to(F16)
    gw, gb = gn_params(C, "sp")
    for up_t in (True, False):
        w_sub, table, ntap = V.subpixel_weights(w.to(DEV), up_t, "fast")
        out, st = V.conv3d_upsampled_subpixel(cl(x), w_sub, table, ntap, b, T, H, W, C, C, up_t, gn_stats=True)
        check(V, out, V.groupnorm_affine_from_stats(st, gw, gb, GROUPS, EPS), gw, gb, what=f"subpixel {data} up_t={up_t}")


def constant_bias(C):
    """0.3, 0.6 or 0.9 (non-dyadic) per group, sign by group: equal within each group"""
    g = torch.arange(C, device=DEV) // (C // GROUPS)
    return (group_sign(C) * 0.3 * (1 + g % 3)).to(F16)


def check_constant(V, out, aff, gb, what):
    """a group of zero variance: rstd = 1/sqrt(eps), GroupNorm returns its bias (to an fp16 ulp, taken at max(|b|, 1/8))"""
    got = V.groupnorm_apply(out, aff, False)
    d = ((got.double() - gb.double()).abs() / fp16_ulp(gb)).max()
    assert float(d) <= 1.0, f"{what}: constant group {float(d):.2f} ulp from its bias"


# the standalone pass's two extreme classes through the epilogue: exactly constant groups (zero weights, non-dyadic bias: C2 = 0
# from the shifted sums; the ragged shapes also leave blocks without a valid row, count 0) and values at the fp16 limit (zero
# weights and bias, the +-(6e4 +- 4e3) data carried by the residual)
@pytest.mark.parametrize("data", ["constant", "fp16max"])
@pytest.mark.parametrize("T,H,W,Cin,Cout", [(3, 6, 5, 64, 64), (2, 7, 12, 128, 128), (3, 5, 16, 128, 64), (2, 6, 10, 256, 256),
                                            (1, 5, 7, 256, 512), (2, 5, 9, 64, 192)])
def test_conv_epilogue_statistics_extremes(V, data, T, H, W, Cin, Cout):
    x = cl(U((1, Cin, T, H, W), "cx.x", device="cpu"))
    wt = torch.zeros(Cout, 27, Cin, dtype=F16, device=DEV)
    if data == "constant":
        b, res = constant_bias(Cout), None
    else:
        b, res = torch.zeros(Cout, dtype=F16, device=DEV), make_x("fp16max", T * H * W, Cout, "cx.res")
    out, st = V.conv3d_causal(x, wt, b, T, H, W, Cin, Cout, res=res, gn_stats=True)
    assert torch.isfinite(out).all()
    gw, gb = gn_params(Cout, "cx")
    aff = V.groupnorm_affine_from_stats(st, gw, gb, GROUPS, EPS)
    check(V, out, aff, gw, gb, what=f"epilogue {data} {Cin}->{Cout}")
    if data == "constant":
        check_constant(V, out, aff, gb, f"epilogue {Cin}->{Cout}")


@pytest.mark.parametrize("data", ["constant", "fp16max"])
def test_subpixel_epilogue_statistics_extremes(V, data):
    """constant: zero weights, non-dyadic bias; fp16 limit: bias +-5e4 with the conv output's std at ~1e3 (R ~ 50, max |y| ~ 5.6e4)"""
    T, H, W, C = 3, 5, 6, 256
    x = U((1, C, T, H, W), "spx.x", device="cpu") * math.sqrt(3.0)
    if data == "constant":
        w, b = torch.zeros(C, C, 3, 3, 3), constant_bias(C)
    else:
        w = U((C, C, 3, 3, 3), "spx.w", device="cpu") * (1e3 * math.sqrt(3.0 / (27 * C)))
        b = (group_sign(C) * 5e4).to(F16)
    gw, gb = gn_params(C, "spx")
    for up_t in (True, False):
        w_sub, table, ntap = V.subpixel_weights(w.to(DEV), up_t, "fast")
        out, st = V.conv3d_upsampled_subpixel(cl(x), w_sub, table, ntap, b, T, H, W, C, C, up_t, gn_stats=True)
        assert torch.isfinite(out).all()
        aff = V.groupnorm_affine_from_stats(st, gw, gb, GROUPS, EPS)
        check(V, out, aff, gw, gb, what=f"subpixel {data} up_t={up_t}")
        if data == "constant":
            check_constant(V, out, aff, gb, f"subpixel up_t={up_t}")


# ---------------------------------------------------------------------------------------------------------------- decoder tail
@pytest.mark.parametrize("kind", ["offset100", "offset1000", "nearconst1", "constant", "control"])
def test_conv_cout4_with_offset_affine(V, kind):
    T, H, W, Cin, Cout = 3, 9, 16, 128, 3
    x = make_x(kind, T * H * W, Cin, f"c4.{kind}")
    gw, gb = gn_params(Cin, "c4")
    w = U((Cout, Cin, 3, 3, 3), "c4.w", device="cpu") * math.sqrt(3.0 / (27 * Cin))
    b = (0.1 * U((Cout,), "c4.b", device="cpu")).to(F16)
    b8 = torch.zeros(8, dtype=F16, device=DEV)
    b8[:Cout] = b.to(DEV)
    aff = V.groupnorm_affine(x, gw, gb, GROUPS, EPS)
    got = V.conv_cout4(x, aff, True, V.cout4_weight_fragments(w.to(DEV)), b8, T, H, W, Cin, Cout)
    # reference: the fp64 definition, SiLU, rounded to fp16 once (the activation the conv reads), then the oracle conv
    mean, rstd, _ = ref_stats(x, Cin)
    y = (x.double() - mean.repeat_interleave(Cin // GROUPS)) * rstd.repeat_interleave(Cin // GROUPS) * gw.double() + gb.double()
    h = (y * torch.sigmoid(y)).to(F16).float().cpu().reshape(T, H, W, Cin).permute(3, 0, 1, 2)[None]
    ref = R.causal_conv3d(h, w.to(F16).float(), b.float(), E)
    got = got[:, :Cout].float().cpu().reshape(T, H, W, Cout).permute(3, 0, 1, 2)[None]
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-3)


# ---------------------------------------------------------------------------------------------------------------- decoder tile
def test_decoder_tile_with_offset_resnet_vs_oracle(monkeypatch):
    """A decoder tile whose first up-block ResNet has conv1 in the offset regime (biases +-15, equal within each group) and a conv2
    bias (+-12) that carries an offset into the residual stream: norm2 (epilogue statistics) and the next norm1 (epilogue statistics
    of a residual conv) see R ~ 30 - 45.  Half the latent is constant.  Same fp16 contract as
    test_gpu_vae.py::test_decoder_tile_vs_reference_golden, at its fp16 drift bound (2e-2) rather than its 5e-3: at R ~ 40 a group is
    only ~R * 2^-10 std per fp16 step wide, so one rounding flip of an offset activation moves its normalised value ~40x more than at
    R ~ 1, and the oracle's own fp16 and fp32 forms of this decode differ by 1.1e-2.  At R ~ 40 one-pass fp32 statistics are still
    within ~1e-4 in rstd, so this test does NOT fail on one-pass statistics (measured: 1.06e-2 with them, 1.11e-2 with the shifted
    ones): it guards the end-to-end path through the regime; the statistics errors are pinned by the kernel-level tests above."""
    from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D
    boc = (64, 64, 128, 128)
    sd = syn.synth_vae_state_dict(boc, seed=0)
    pre = "decoder.up_blocks.0.resnets.0."
    co = sd[pre + "conv1.conv.bias"].shape[0]
    g = torch.arange(co) // (co // GROUPS)
    sgn = torch.where((g % 4) < 2, 1.0, -1.0)
    sd[pre + "conv1.conv.bias"] = sgn * (15.0 + 0.5 * syn.hashed_uniform((GROUPS,), "dt.b1", 0)[g])
    sd[pre + "conv2.conv.bias"] = sgn * (12.0 + 0.5 * syn.hashed_uniform((GROUPS,), "dt.b2", 0)[g])
    vae = AutoencoderKLCausal3D(block_out_channels=boc, sample_size=256, sample_tsize=64, device=DEV)
    vae.load_state_dict({k: v.to(F16) for k, v in sd.items()}, strict=True)
    sd16 = {k: v.to(F16).float() for k, v in sd.items()}
    z = syn.hashed_uniform((1, 16, 3, 8, 8), "dt.z", 0) * 1.7
    z[..., :, 4:] = 0.6                                                         # constant over half the tile

    seen = []
    gn = R.group_norm_silu

    def recording(x, w, b, groups=32, eps=1e-6, silu=True):
        xg = x.double().reshape(x.shape[0], groups, -1)
        seen.append(float((xg.mean(-1).abs() / torch.sqrt(xg.var(-1, unbiased=False) + eps)).max()))
        return gn(x, w, b, groups, eps, silu)

    monkeypatch.setattr(R, "group_norm_silu", recording)
    ref16 = R.decode_tile(sd16, z, boc, E)
    assert max(seen) >= 30.0, f"no GroupNorm input reached R >= 30 (max {max(seen):.1f}): the test no longer exercises the regime"
    y = vae.decode(z.to(DEV), return_dict=False)[0]
    rel = float((y.float().cpu() - ref16).abs().max() / ref16.abs().max())
    assert rel < 2e-2, rel


# ---------------------------------------------------------------------------------------------------------------- DiT norms
def dit_rows(M, D, key):
    """bf16 rows: DiT-style massive activations (a few channels at +-1000..3000), a row offset by 500 (std 1), a constant row, the
    rest N(0, 1)-like"""
    u = syn.hashed_uniform((M, D), key, 9) * math.sqrt(3.0)
    x = u.clone()
    x[0, [3, D // 2, D - 5]] = torch.tensor([2800.0, -1500.0, 1000.0])
    x[1, 17] = -3000.0
    x[1, 400 % D] = 2000.0
    x[2] = 500.0 + u[2]
    x[3] = 0.3
    x[4] = -500.0 + u[4]
    return x.to(torch.bfloat16)


def ln_ref(x, shift, scale, w=None, b=None, eps=1e-6):
    """fp64 LayerNorm (+ modulate with bf16(1 + scale), or the affine) of bf16 rows, rounded to bf16"""
    xd = x.double()
    y = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + eps)
    if w is not None:
        y = y * w.double() + b.double()
    else:
        y = y * (1.0 + scale.double()).to(torch.bfloat16).double() + shift.double()
    return y.to(torch.bfloat16)


@pytest.mark.parametrize("M,D", [(8, 3072), (6, 256)])
def test_dit_layernorm_conditioning(M, D):
    from hunyuanvideo_efficiency_amd import ops
    x = dit_rows(M, D, f"dl.{D}")
    sh = (syn.hashed_uniform((D,), "dl.sh", 9) * 0.5).to(torch.bfloat16)
    sc = (syn.hashed_uniform((D,), "dl.sc", 9) * 0.5).to(torch.bfloat16)
    close = lambda got, ref: torch.testing.assert_close(got.float().cpu(), ref.float(), rtol=2 ** -7, atol=2e-2)
    close(ops.ln_modulate(x.to(DEV), sh.to(DEV), sc.to(DEV)), ln_ref(x, sh, sc))
    w, b = (1 + 0.1 * syn.hashed_uniform((D,), "dl.w", 9)).to(torch.bfloat16), sh
    close(ops.ln_modulate(x.to(DEV), b.to(DEV), w.to(DEV), affine=True), ln_ref(x, None, None, w, b))
    # FP8 form: the same LayerNorm, quantised per row (contract of test_gpu_fp8_mfma.py::test_quantisers_bit_exact)
    from oracle import dit_ref as DR
    q_ref, s_ref = DR.fp8_quant_rows(ln_ref(x, sh, sc).float())
    q, s = ops.ln_modulate_fp8(x.to(DEV), sh.to(DEV), sc.to(DEV))
    torch.testing.assert_close(s.cpu(), s_ref[:, 0], rtol=2 ** -7, atol=0)
    deq, deq_ref = q.cpu().float() * s.cpu()[:, None], q_ref * s_ref
    assert float((deq - deq_ref).abs().max()) <= float(s_ref.max()) * 32.0 + 1e-6
    assert float(((deq - deq_ref).abs() > 1e-6).float().mean()) < 0.05


def test_dit_qknorm_conditioning():
    from hunyuanvideo_efficiency_amd import ops
    H, n_rows, n_rope = 2, 8, 6
    ld = 3 * H * 128
    qkv = dit_rows(n_rows, ld, "dq")
    qw = (1 + 0.1 * syn.hashed_uniform((128,), "dq.qw", 9)).to(torch.bfloat16)
    kw = (1 + 0.1 * syn.hashed_uniform((128,), "dq.kw", 9)).to(torch.bfloat16)
    ang = syn.hashed_uniform((n_rope, 64), "dq.ang", 9) * 3.0
    cos, sin = ang.cos().repeat_interleave(2, 1).contiguous(), ang.sin().repeat_interleave(2, 1).contiguous()
    got = ops.qknorm_rope_(qkv.to(DEV), qw.to(DEV), kw.to(DEV), cos.to(DEV), sin.to(DEV), n_rope, H, H * 128).float().cpu()
    # fp64 RMSNorm per head, rounded to bf16, times the gain (rounded), then RoPE on the first n_rope rows in fp64, rounded once
    heads = qkv.double().reshape(n_rows, 3, H, 128)
    gain = torch.stack([qw, kw]).double()[:, None, :]
    r = heads[:, :2] / torch.sqrt((heads[:, :2] ** 2).mean(-1, keepdim=True) + 1e-6)
    r = (r.to(torch.bfloat16).double() * gain).to(torch.bfloat16).double()
    x0, x1 = r[..., 0::2], r[..., 1::2]
    rot = torch.stack([-x1, x0], -1).flatten(-2)
    rr = r.clone()
    rr[:n_rope] = r[:n_rope] * cos.double()[:, None, None, :] + rot[:n_rope] * sin.double()[:, None, None, :]
    ref = torch.cat([rr.to(torch.bfloat16).float().reshape(n_rows, 2 * H * 128), qkv[:, 2 * H * 128:].float()], 1)
    torch.testing.assert_close(got, ref, rtol=2 ** -7, atol=2e-2)
