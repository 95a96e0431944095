"""fp64 references and per-element error bounds of the conv entry points, in the conventions of tests/error_bounds.py (a kernel that
multiplies fp16 operands exactly and accumulates in fp32 in any order: ulp_out(y64) + C sqrt(K) 2^-24 P, C = 4).

conv_ref: the implicit GEMM of hv_conv3d_causal_f16 and hv_conv3d_causal_strided_f16 (K = 27 Cin), gathered by the padding rule of
include/hv_kernels.h: output voxel (t, h, w), tap (dt, dh, dw) reads source
    (max(t st + dt - 2, 0), clamp(h sh + dh - 1, 0, bH - 1), clamp(w sw + dw - 1, 0, bW - 1)),
bH / bW the SOURCE extents (as the nearest upsample shows them: sH << up_hw), then the upsample's halvings.

cout4_ref: hv_conv3d_cout4_f16 (GroupNorm affine [+ SiLU] + conv_out), from the header's contract:
    h64 = [silu](x scale + shift) per element, or x itself without an affine;  h = fp16(h64);
    y64 = bias + sum over 27 taps and Cin of w h at the clamped tap-shifted voxel (conv_ref's rule, unit stride).
The kernel evaluates h64 in fp32 (rowwise_bounds.gn_apply_eval states the error e32 of that evaluation) before the one rounding to
fp16.  Where h64 lies within e32 of an fp16 rounding boundary (the midpoint of two neighbouring fp16 values) the kernel may round the
other way: such a (voxel, channel) is AMBIGUOUS, as in rowwise_bounds.qknorm_ref, and adds |w| ulp_fp16(h) to the bound of every
output that reads it.  An unambiguous element adds nothing: its fp16 value is known exactly.
    bound = ulp_fp16(y64) + C sqrt(27 Cin) 2^-24 P + sum over ambiguous operands |w| ulp_fp16(h)
The mask must stay a small share of the data or it could hide a failure: cout4_act returns the share, and every test asserts it is at
most 1 % (measured on the inputs of the GPU test, tests/test_conv_bounds_cpu.py: up to 0.87 % with SiLU - its negative branch gives small
values with the absolute error of the affine -, 0.30 % affine only).

tests/test_conv_bounds_cpu.py shows what the bounds accept (fp32 emulations in the planes-then-gather order, as one 27 Cin sum and
in reversed order) and what they reject (a dropped tap plane, a clamp at W - 2, a replicate clamp at the far end of T, the activation
rounded to fp16 in front of the SiLU, a strided clamp at the output extent, a t coordinate wrapped & 255)."""
from __future__ import annotations

import math

import torch

from tests import error_bounds as EB
from tests import rowwise_bounds as RB

F16 = torch.float16
AMBIGUOUS_SHARE_LIMIT = 0.01


def src_rows(m, tap, oH, oW, src, stride=(1, 1, 1), up_t=False, up_hw=False):
    """source row of tap (dt, dh, dw) = (tap / 9, tap / 3 % 3, tap % 3) for the output rows m of a [., oH, oW] grid; src = (sT, sH, sW)"""
    _, sH, sW = src
    st, sh, sw = stride
    bH, bW = sH << int(up_hw), sW << int(up_hw)
    t, h, w = m // (oH * oW), (m // oW) % oH, m % oW
    dt_, dh, dw = tap // 9, (tap // 3) % 3, tap % 3
    ti = (t * st + dt_ - 2).clamp(min=0)
    if up_t:
        ti = torch.where(ti == 0, ti, 1 + (ti - 1) // 2)
    hi = (h * sh + dh - 1).clamp(0, bH - 1) >> int(up_hw)
    wi = (w * sw + dw - 1).clamp(0, bW - 1) >> int(up_hw)
    return (ti * sH + hi) * sW + wi


def out_grid(src, stride):
    return tuple((s - 1) // m + 1 for s, m in zip(src, stride))


def conv_ref(x, w_taps, b, T, H, W, cin, cout, up_t=False, up_hw=False, stride=(1, 1, 1), src=None) -> EB.Ref:
    """fp64 im2col reference over the OUTPUT grid T x H x W.  src: the source extents (sT, sH, sW); without it the unit-stride source of
    hv_conv3d_causal_f16, ((T + 1) / 2 if up_t else T, H >> up_hw, W >> up_hw).  x: the source rows [sT sH sW, >= cin]."""
    if src is None:
        src = ((T + 1) // 2 if up_t else T, H >> int(up_hw), W >> int(up_hw))
    m = torch.arange(T * H * W, device=x.device)
    wt = w_taps.reshape(cout, 27, cin)
    ref = EB.Ref()
    for tap in range(27):
        ref.add(x[src_rows(m, tap, H, W, src, stride, up_t, up_hw)][:, :cin], wt[:, tap])
    return ref.bias(b)


# ---------------------------------------------------------------------------------------------------- hv_conv3d_cout4_f16
def near_f16_boundary(h64, e):
    """h64 within e of the midpoint of two neighbouring fp16 values (subnormal spacing 2^-24 below the smallest normal)"""
    u = EB.ulp_out(h64, F16)
    frac = h64.abs() / u
    return ((frac - torch.floor(frac)) - 0.5).abs() * u <= e


def cout4_act(x, affine, silu: bool):
    """x [M, Cin] fp16, affine fp32 [Cin, 2] or None -> (h, au, share): the fp16 activation the conv reads, as fp64 values; au =
    ulp_fp16(h) where the element is ambiguous and 0 elsewhere (None without an affine: h is x); the ambiguous share"""
    if affine is None:
        return x.double(), None, 0.0
    h64, e32 = RB.gn_apply_eval(x, affine, silu)
    h = h64.to(F16).double()
    amb = near_f16_boundary(h64, e32)
    return h, torch.where(amb, EB.ulp_out(h, F16), torch.zeros_like(h)), float(amb.double().mean())


def cout4_ref(h, au, w, b, T, H, W, r0=0, r1=None):
    """(y64, bound) of the output rows [r0, r1) from cout4_act's (h, au); w [Cout, Cin, 3, 3, 3], b [Cout] fp16"""
    cout, cin = w.shape[:2]
    wt = w.double().permute(0, 2, 3, 4, 1).reshape(cout, 27, cin)
    m = torch.arange(r0, T * H * W if r1 is None else r1, device=h.device)
    ref, extra = EB.Ref(), 0.0
    for tap in range(27):
        s = src_rows(m, tap, H, W, (T, H, W))
        ref.add(h[s], wt[:, tap])
        if au is not None:
            extra = extra + au[s] @ wt[:, tap].abs().T
    ref.bias(b)
    return ref.y, ref.bound(F16) + extra


def cout4_operands(M, cin, cout, key, dev="cpu"):
    """the inputs every cout4 test uses (the 1 % ambiguity condition is confirmed on them on the CPU): x hashed uniform (unit variance) fp16,
    scale 1 +- 0.5, shift +- 1, weights of std 1 / sqrt(27 Cin), bias +- 0.1"""
    from hunyuanvideo_efficiency_amd import synthetic as syn

    def u(shape, k, scale=1.0):
        return syn.hashed_uniform(shape, f"{key}.{k}", 47, dev) * (scale * math.sqrt(3.0))

    x = u((M, cin), "x").to(F16)
    aff = torch.stack([1.0 + u((cin,), "sc", 0.5 / math.sqrt(3.0)), u((cin,), "sh", 1.0 / math.sqrt(3.0))], 1).contiguous()
    w = u((cout, cin, 3, 3, 3), "w", 1.0 / math.sqrt(27 * cin)).to(F16)
    b = u((cout,), "b", 0.1 / math.sqrt(3.0)).to(F16)
    return x, aff, w, b


COUT4_MODES = {"affine+silu": (True, True), "affine": (True, False), "plain": (False, False)}
COUT4_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 4, 6), (1, 4, 9), (3, 1, 5), (3, 4, 1)]      # 105 voxels: a ragged 16-voxel group; 48: M % 16 == 0;
COUT4_CINS = [32, 64, 96, 128]                                                         # T = 1, H = 1, W = 1: every tap of one axis clamps
COUT4_CAP = [(3, 209, 210), (5, 229, 230)]      # 131,670 voxels: a second grid-stride trip for some waves; 263,350: a third (the prefetch)


def cout4_cases():
    """(T, H, W, Cin, Cout, ldo, mode): every Cin at every shape; every (Cout, ldo) and every (mode, ldo) pair"""
    modes, ldos, couts = list(COUT4_MODES), [3, 8, 16], [3, 1, 2]
    cases = []
    for cin in COUT4_CINS:
        for shp in COUT4_SHAPES:
            i = len(cases)
            cases.append((*shp, cin, couts[i % 3], ldos[(i // 3) % 3], modes[(i + i // 9) % 3]))
    assert {(c[4], c[5]) for c in cases} == {(a, b) for a in couts for b in ldos}
    assert {(c[6], c[5]) for c in cases} == {(a, b) for a in modes for b in ldos}
    return cases


def cout4_key(T, H, W, cin, cout):
    """the hash key of a case's operands.  A one-voxel case has 32 .. 128 activations, so a single ambiguous one is above the 1 % limit: the
    salt (2) is the first for which every case of cout4_cases stays within it (tests/test_conv_bounds_cpu.py asserts that)"""
    return f"c4.2.{T}.{H}.{W}.{cin}.{cout}"
