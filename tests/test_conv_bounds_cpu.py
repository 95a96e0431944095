"""CPU: the bounds of tests/conv_bounds.py have teeth.  fp32 emulations of hv_conv3d_cout4_f16 in three summation orders (the kernel's
planes-then-gather order - the CPU double of tests/cpu_kernel_doubles.py -, one direct 27 Cin sum, the reversed order) are accepted; the
ways the kernel or its gather can be subtly wrong are rejected (at least one element outside the bound).  The strided reference is
compared with the oracle's own padding + strided Conv3d in fp64, and the 1 % ambiguity condition is asserted on the inputs of the GPU
test (tests/test_gpu_conv_out_edges.py takes them from the same conv_bounds.cout4_operands).

Largest error-to-bound ratio the faithful emulations reach over every case of the GPU test, every mode at each
(test_cout4_faithful_accepted_and_ambiguity_below_one_percent prints them):
    affine + SiLU 0.525    affine only 0.492    no affine 0.486
Largest ambiguous share of the activations of a case: 0.0087 with SiLU, 0.0030 affine only (limit 0.01); the grid-cap cases 0.0059 /
0.0022 (131,670 voxels) and 0.0053 / 0.0018 (263,350)."""
import math

import pytest
import torch

from hunyuanvideo_efficiency_amd import synthetic as syn
from hunyuanvideo_efficiency_amd import vae_ops
from oracle import vae_enc_ref as VE
from oracle import vae_ref as VR
from tests import conv_bounds as CB
from tests import cpu_kernel_doubles as KD
from tests import error_bounds as EB
from tests import rowwise_bounds as RB

F16, F32 = torch.float16, torch.float32


def silu32(t):
    return t / (1.0 + torch.exp(-t))


def gather(m, tap, oH, oW, src, stride=(1, 1, 1), mutant=None):
    """the index rule, written on its own (not conv_bounds.src_rows), with the ways to get it wrong"""
    sT, sH, sW = src
    t, h, w = m // (oH * oW), (m // oW) % oH, m % oW
    dt, dh, dw = tap // 9, (tap // 3) % 3, tap % 3
    tc = t * stride[0]
    if mutant == "t_wrapped":
        tc = tc & 255
    ti = (tc + dt - 2).clamp(min=0)
    if mutant == "t_replicate":                       # a replicate clamp at the far end in place of the causal front pad: (t + dt - 1)
        ti = (tc + dt - 1).clamp(0, sT - 1)
    hb, wb = sH - 1, sW - 1
    if mutant == "w_minus_2":
        wb = max(sW - 2, 0)
    if mutant == "output_extent":                     # the clamp at the output extent instead of the source extent
        hb, wb = oH - 1, oW - 1
    hi = (h * stride[1] + dh - 1).clamp(0, hb)
    wi = (w * stride[2] + dw - 1).clamp(0, wb)
    return (ti * sH + hi) * sW + wi


def cout4_emul(x, aff, silu, w, b, T, H, W, order="planes", mutant=None):
    cout, cin = w.shape[:2]
    M = T * H * W
    h = x.float()
    if aff is not None:
        t = h * aff[:, 0][None] + aff[:, 1][None]
        if mutant == "act_rounded_before_silu":
            t = t.to(F16).float()
        h = silu32(t) if silu else t
    h = h.to(F16).float()
    wt = w.float().permute(0, 2, 3, 4, 1).reshape(cout, 27, cin)
    m = torch.arange(M)
    taps = [tp for tp in range(27) if not (mutant == "drop_plane" and tp == 13)]
    if order == "direct":
        a = torch.cat([h[gather(m, tp, H, W, (T, H, W), mutant=mutant)] for tp in taps], 1)
        acc = a @ torch.cat([wt[:, tp] for tp in taps], 1).T + b.float()[None]
    elif order == "reversed":
        acc = torch.zeros(M, cout)
        for tp in reversed(taps):
            acc = acc + h[gather(m, tp, H, W, (T, H, W), mutant=mutant)].flip(1) @ wt[:, tp].flip(1).T
        acc = acc + b.float()[None]
    else:
        acc = b.float()[None].expand(M, cout).clone()
        for tp in taps:
            plane = torch.zeros(M, cout)
            for k0 in range(0, cin, 32):
                plane = plane + h[:, k0:k0 + 32] @ wt[:, tp, k0:k0 + 32].T
            acc = acc + plane[gather(m, tp, H, W, (T, H, W), mutant=mutant)]
    return acc.to(F16)


def _case(T, H, W, cin, cout, mode):
    x, aff, w, b = CB.cout4_operands(T * H * W, cin, cout, CB.cout4_key(T, H, W, cin, cout))
    with_aff, silu = CB.COUT4_MODES[mode]
    aff = aff if with_aff else None
    h, au, share = CB.cout4_act(x, aff, silu)
    y, bound = CB.cout4_ref(h, au, w, b, T, H, W)
    return x, aff, silu, w, b, y, bound, share


def outside(got, y, bound):
    return int((RB.ratio(got, y, bound) > 1.0).sum())


def test_cout4_faithful_accepted_and_ambiguity_below_one_percent(capsys):
    """every case of the GPU test (the same operands), every mode at each, in the three orders and through the CPU double"""
    worst, worst_share = {m: 0.0 for m in CB.COUT4_MODES}, {m: 0.0 for m in CB.COUT4_MODES}
    for T, H, W, cin, cout, _, case_mode in CB.cout4_cases():
        for mode in CB.COUT4_MODES:
            x, aff, silu, w, b, y, bound, share = _case(T, H, W, cin, cout, mode)
            if mode == case_mode:
                assert share <= CB.AMBIGUOUS_SHARE_LIMIT, (mode, cin, T, H, W, share)
                worst_share[mode] = max(worst_share[mode], share)
            what = f"{mode} {cin}->{cout} {T}x{H}x{W}"
            for order in ("planes", "direct", "reversed"):
                worst[mode] = max(worst[mode], RB.check(cout4_emul(x, aff, silu, w, b, T, H, W, order), y, bound, f"{what} {order}"))
            got = KD.conv_cout4(x, aff, silu, vae_ops.cout4_weight_fragments(w), b, T, H, W, cin, cout)
            assert float(got[:, cout:].abs().max()) == 0.0
            worst[mode] = max(worst[mode], RB.check(got[:, :cout], y, bound, f"{what} double"))
    with capsys.disabled():
        print("\ncout4 faithful emulations, largest |got - y64| / bound: " + ", ".join(f"{m} {r:.3f}" for m, r in worst.items())
              + "; largest ambiguous share: " + ", ".join(f"{m} {s:.4f}" for m, s in worst_share.items()))
    assert all(0.05 < r <= 1.0 for r in worst.values()), worst


def test_ambiguous_share_of_the_grid_cap_inputs():
    """the activations of the two grid-cap cases of the GPU test, whole"""
    for T, H, W in CB.COUT4_CAP:
        x, aff, _, _ = CB.cout4_operands(T * H * W, 128, 3, CB.cout4_key(T, H, W, 128, 3))
        for silu in (True, False):
            _, au, share = CB.cout4_act(x, aff, silu)
            assert 0.0 < share <= CB.AMBIGUOUS_SHARE_LIMIT, (T, H, W, silu, share)


@pytest.mark.parametrize("mutant", ["drop_plane", "w_minus_2", "t_replicate", "act_rounded_before_silu"])
def test_cout4_mutants_rejected(mutant):
    T, H, W, cin = 3, 5, 7, 128
    for mode in (("affine+silu",) if mutant == "act_rounded_before_silu" else ("affine+silu", "plain")):
        x, aff, silu, w, b, y, bound, _ = _case(T, H, W, cin, 3, mode)
        for order in ("planes", "direct"):
            assert outside(cout4_emul(x, aff, silu, w, b, T, H, W, order), y, bound) == 0
            assert outside(cout4_emul(x, aff, silu, w, b, T, H, W, order, mutant=mutant), y, bound) > 0, (mutant, mode, order)


def test_fragment_order_round_trip():
    w = syn.hashed_uniform((3, 96, 3, 3, 3), "frag", 5).to(F16)
    wn = KD.cout4_weights_from_fragments(vae_ops.cout4_weight_fragments(w))
    assert torch.equal(wn[:27, :3, :96], w.reshape(3, 96, 27).permute(2, 0, 1))
    assert float(wn[27:].abs().max()) == 0.0 and float(wn[:, 3].abs().max()) == 0.0 and float(wn[:, :, 96:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- the strided reference
def _strided_operands(src, cin, cout, key):
    n = src[0] * src[1] * src[2]
    x = (syn.hashed_uniform((n, cin), key + ".x", 17) * math.sqrt(3.0)).to(F16)
    w = (syn.hashed_uniform((cout, 27 * cin), key + ".w", 17) * math.sqrt(3.0 / (27 * cin))).to(F16)
    b = (syn.hashed_uniform((cout,), key + ".b", 17) * 0.1).to(F16)
    return x, w, b


def strided_emul(x, w, b, src, cin, cout, stride, mutant=None):
    T, H, W = CB.out_grid(src, stride)
    m = torch.arange(T * H * W)
    wt = w.float().reshape(cout, 27, cin)
    acc = torch.zeros(T * H * W, cout)
    for tap in range(27):
        acc = acc + x[gather(m, tap, H, W, src, stride, mutant)].float() @ wt[:, tap].T
    return (acc + b.float()[None]).to(F16)


STRIDES = [(2, 2, 2), (1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 2), (1, 2, 1), (2, 1, 1), (1, 1, 1)]


@pytest.mark.parametrize("stride", STRIDES, ids=["".join(map(str, s)) for s in STRIDES])
def test_strided_reference_matches_the_oracle_in_fp64(stride):
    for src in [(1, 1, 1), (2, 2, 2), (5, 7, 9), (4, 6, 8), (3, 6, 5)]:
        cin, cout = 64, 8
        x, w, b = _strided_operands(src, cin, cout, f"so.{src}")
        T, H, W = CB.out_grid(src, stride)
        ref = CB.conv_ref(x, w, b, T, H, W, cin, cout, stride=stride, src=src)
        x5 = x.double().reshape(*src, cin).permute(3, 0, 1, 2)[None]
        w5 = w.double().reshape(cout, 3, 3, 3, cin).permute(0, 4, 1, 2, 3)
        o5 = VE.causal_conv3d_strided(x5, w5, b.double(), stride, VR.FP32)
        assert tuple(o5.shape[2:]) == (T, H, W)
        torch.testing.assert_close(ref.y, o5[0].permute(1, 2, 3, 0).reshape(T * H * W, cout), rtol=1e-12, atol=1e-12)
        got, T2, H2, W2 = KD.conv3d_causal_strided(x, w, b, *src, cin, cout, stride)
        assert (T2, H2, W2) == (T, H, W)
        assert float(EB.ratio(got, ref, F16).max()) <= 1.0, (src, stride)
        assert float(EB.ratio(strided_emul(x, w, b, src, cin, cout, stride), ref, F16).max()) <= 1.0, (src, stride)


def test_strided_clamp_at_the_output_extent_rejected():
    """an odd source extent with a stride of 2: the last output column reads one past the source and clamps at sW - 1, far beyond oW - 1"""
    src, cin, cout = (3, 7, 9), 64, 8
    x, w, b = _strided_operands(src, cin, cout, "sm")
    for stride in [(2, 2, 2), (1, 2, 1), (1, 1, 2)]:
        T, H, W = CB.out_grid(src, stride)
        ref = CB.conv_ref(x, w, b, T, H, W, cin, cout, stride=stride, src=src)
        assert float(EB.ratio(strided_emul(x, w, b, src, cin, cout, stride), ref, F16).max()) <= 1.0
        assert float(EB.ratio(strided_emul(x, w, b, src, cin, cout, stride, "output_extent"), ref, F16).max()) > 1.0, stride


def test_wrapped_t_coordinate_rejected():
    """T = 257 frames of 1 x 2 voxels: a t coordinate kept in 8 bits wraps at frame 256"""
    src, cin, cout = (257, 1, 2), 64, 8
    x, w, b = _strided_operands(src, cin, cout, "wrap")
    ref = CB.conv_ref(x, w, b, *src, cin, cout)
    r = EB.ratio(strided_emul(x, w, b, src, cin, cout, (1, 1, 1), "t_wrapped"), ref, F16)
    assert float(EB.ratio(strided_emul(x, w, b, src, cin, cout, (1, 1, 1)), ref, F16).max()) <= 1.0
    assert float(r[:256 * 2].max()) <= 1.0 and float(r[256 * 2:].min()) > 1.0
