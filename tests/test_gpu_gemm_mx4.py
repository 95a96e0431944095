"""GPU: the opt-in MXFP4 linears (include/hv_gemm_mx4.h) against tests/mxfp4_ref.py, the torch restatement of that header.

(1) operand and scale maps of v_mfma_scale_f32_16x16x128_f8f6f4 as the kernel feeds it: exactly representable data, every partial sum
exact in fp32, so the output is the bf16 rounding of the fp64 product, bit for bit; (2) both quantisers bit for bit; (3) the GEMM on
random data given the same quantised operands, element by element inside tests/error_bounds.py's worst-case form (the one it prescribes
for the scaled MFMA), at every K-stage count the loop distinguishes - K / 128 = 4 (the minimum: the tail alone) .. 9 (one past the
ring period 4 and the unroll 2, with and without the peeled front iteration) - and at K = 15360; (4) a d = 512 model against the
quantisation-aware oracle.  Measured worst error / bound in (3): see README.  Measured on one MI355X in (4): see the docstring there."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import error_bounds as EB  # noqa: E402
from tests import mxfp4_ref as MX  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402

DEV = "cuda"
E = R.Prec(True)
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    """the MXFP4 wrappers (hunyuanvideo_efficiency_amd.gemm_mx4, with the activation constants of ops)"""
    from hunyuanvideo_efficiency_amd import gemm_mx4, _lib
    _lib.torch_ops()
    return gemm_mx4


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 23) * (scale * math.sqrt(3.0))


def test_operand_and_scale_maps_exact(ops):
    """codes and scales that differ along m, n, k and per (row, block): a swapped nibble pairing, a scale from the wrong k-block or row,
    or a wrong op_sel byte changes the result.  |products| <= 36 * 2^6 in units of 2^-8, K = 1024: every partial sum fits 24 bits."""
    M, N, K = 300, 264, 1024
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    ca, cw = (m * 7 + k * 3 + (k // 32) * 5) % 16, (n * 5 + k * 11 + (k // 64)) % 16
    pack = lambda c: (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)
    blk = torch.arange(K // 32)[None, :]
    sa, sw = (126 + (m * 3 + blk) % 4).to(torch.uint8), (126 + (n + 2 * blk) % 4).to(torch.uint8)
    b = ((torch.arange(N) % 7) - 3).float()
    ref = (MX.dequant(pack(ca), sa).double() @ MX.dequant(pack(cw), sw).double().T + b.double()).to(BF)
    got = ops.gemm_mxfp4(pack(ca).to(DEV), sa.to(DEV), pack(cw).to(DEV), sw.to(DEV), b.to(BF).to(DEV))
    assert torch.equal(got.cpu(), ref)


def _edge_rows(M, K):
    """random rows whose first blocks are the contract's edge cases: zero; maximum a power of two; maximum just below one (saturates at
    6); ties at 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 times the scale, both signs; subnormals only"""
    x = U((M, K), f"q.x{M}.{K}", 2.0).to(BF)
    x[:, 0:32] = 0
    x[:, 32:64] = (U((M, 32), "q.p2", 1.0).clamp(-3.9, 3.9)).to(BF)
    x[:, 40] = 4.0
    x[:, 64:96] = x[:, 32:64]
    x[:, 72] = -3.984375
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 0.0, 6.0]) * 2.0 ** -3
    x[:, 96:128] = torch.cat([ties, ties.flip(0)]).to(BF)
    x[:, 100] = 5.0 * 2.0 ** -3                       # (the block's maximum must stay 6 * 2^-3 or 5 * 2^-3: both have the same exponent)
    sub = ((torch.arange(32) * 4 + 1) % 128).to(torch.int16)
    sub[1::2] |= -32768
    x[:, 128:160] = sub.view(BF)
    return x


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("K", [512, 2560])
def test_quantisers_bit_exact(ops, M, K):
    x = _edge_rows(M, K)
    c_ref, s_ref = MX.quant_rows(x)
    c, s = ops.quant_rows_mxfp4(x.to(DEV))
    assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref)
    assert int(s_ref[0, 0]) == 0 and int(c_ref[0, :16].max()) == 0 and int(s_ref[0, 4]) == 0 and int(c_ref[0, 64:80].max()) > 0
    wide = torch.zeros(M, K + 512, dtype=BF, device=DEV)          # strided input: a column slice of a wider buffer, as cat[:, d:]
    wide[:, 512:] = x.to(DEV)
    c, s = ops.quant_rows_mxfp4(wide[:, 512:])
    assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref)
    # fused LayerNorm: the kernel's statistics are fp32 sums in its own order, so its bf16 LayerNorm output may sit one ulp from the
    # restatement's on a few elements, and only there may a code differ.  CAP bounds that share; the restatement itself, run in two
    # summation orders (fp32 and fp64 statistics), must stay inside it on these inputs.
    CAP = 0.02
    xr = U((M, K), f"q.ln{M}.{K}", 2.0).to(BF)
    sh, sc = U((K,), "q.sh", 0.3).to(BF), U((K,), "q.sc", 0.3).to(BF)
    y = E.r(R.ln_modulate(xr.float()[None], sh.float()[None], sc.float()[None], E))[0]
    x64 = xr.double()
    n64 = (x64 - x64.mean(-1, keepdim=True)) / (x64.var(-1, unbiased=False, keepdim=True) + 1e-6).sqrt()
    y64 = E.r((n64.float() * E.r(1.0 + sc.float()) + sh.float()))
    c_ref, s_ref = MX.quant_rows(y)
    assert float((MX.quant_rows(y64)[0] != c_ref).float().mean()) < CAP
    c, s = ops.ln_modulate_mxfp4(xr.to(DEV), sh.to(DEV), sc.to(DEV))
    assert torch.equal(s.cpu(), s_ref)
    share = float((c.cpu() != c_ref).float().mean())
    print(f"ln_modulate_mxfp4 M={M} K={K}: share of code bytes that differ {share:.4f}")
    assert share < CAP


WORST = {}


def _check_gemm(ops, a, w, b, M, N, K):
    """the kernel on the first M rows of a and N rows of w, quantised by the kernel's own quantiser, against fp64 over the dequantised
    operands; then the epilogues, exactly, against the oracle's formulas applied to the kernel's own y"""
    a4, a4s = ops.quant_rows_mxfp4(a[:M].to(DEV))
    w4, w4s = ops.quant_rows_mxfp4(w[:N].to(DEV))
    bd = b[:N].to(DEV)
    got = ops.gemm_mxfp4(a4, a4s, w4, w4s, bd)
    ref = EB.gemm_ref(MX.dequant(a4, a4s), MX.dequant(w4, w4s), b[:N].float())
    WORST[K] = max(WORST.get(K, 0.0), EB.check(got.cpu(), ref, BF, f"gemm_mxfp4 {M}x{N}x{K}", worst_case=True))
    y = got.float().cpu()
    got = ops.gemm_mxfp4(a4, a4s, w4, w4s, bd, act=ops.ACT_GELU_TANH)
    torch.testing.assert_close(got.float().cpu(), R.gelu_tanh(y, E), rtol=2 ** -7, atol=2e-2)       # (GELU: exp2-based tanh vs torch's)
    gate, res = U((N,), "f.g", 0.5).to(BF), U((M, N), "f.r").to(BF)
    r_dev = res.to(DEV).clone()
    got = ops.gemm_mxfp4(a4, a4s, w4, w4s, bd, out=r_dev, gate=gate.to(DEV), res=r_dev)
    assert torch.equal(got.float().cpu(), R.gate_residual(res.float()[None], y[None], gate.float()[None], E)[0])
    if N >= 16:
        ns = (N // 2) // 8 * 8                  # column split (linear1's qkv | mlp) with act1 on the second part
        out0 = torch.zeros(M, ns + 64, dtype=BF, device=DEV)
        out1 = torch.zeros(M, N, dtype=BF, device=DEV)
        ops.gemm_mxfp4(a4, a4s, w4, w4s, bd, out=out0, n_split=ns, out1=out1[:, 8:], act1=ops.ACT_GELU_TANH)
        assert torch.equal(out0[:, :ns].float().cpu(), y[:, :ns]) and float(out0[:, ns:].abs().max()) == 0
        torch.testing.assert_close(out1[:, 8:8 + N - ns].float().cpu(), R.gelu_tanh(y[:, ns:], E), rtol=2 ** -7, atol=2e-2)
        assert float(out1[:, :8].abs().max()) == 0


@pytest.mark.parametrize("K", [512, 640, 768, 896, 1024, 1152])
def test_gemm_random_same_operands(ops, K):
    a, w, b = U((300, K), f"f.a{K}", 1.5).to(BF), U((520, K), f"f.w{K}", 1.0).to(BF), U((520,), "f.b", 0.1).to(BF)
    for M in (1, 257, 300):
        for N in (8, 264, 520):
            _check_gemm(ops, a, w, b, M, N, K)
    print(f"gemm_mxfp4 K={K}: worst error / bound {WORST[K]:.3f}")


def test_gemm_production_depth(ops):
    K = 15360
    a, w, b = U((33, K), "f.a15", 1.5).to(BF), U((72, K), "f.w15", 1.0).to(BF), U((72,), "f.b", 0.1).to(BF)
    _check_gemm(ops, a, w, b, 33, 72, K)
    print(f"gemm_mxfp4 K={K}: worst error / bound {WORST[K]:.3f}")


def test_model_mxfp4_vs_quantisation_aware_oracle():
    """Measured on one MI355X: see README (MXFP4 linears)."""
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.mxfp4_optimization import convert_mxfp4_linear, enable_mxfp4_linears
    from hunyuanvideo_efficiency_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    model = build_model(cfg, DEV)
    sd_bf16 = {k: p.float().cpu() for k, p in model.state_dict().items()}
    assert convert_mxfp4_linear(model) == 8 + 2 * 2 and enable_mxfp4_linears(model) == 3
    with pytest.raises(RuntimeError, match="mxfp4"):
        model.single_blocks[0].linear1.w()
    thw, txt_len, n_valid = (5, 16, 16), 32, 11
    x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, thw, txt_len, n_valid, seed=2)
    T, H, W = thw
    cos, sin = get_nd_rotary_pos_embed(cfg.rope_dim_list, [T, H // 2, W // 2], theta=256, use_real=True)
    g, t = torch.tensor([6016.0]), torch.tensor([997.093])
    with torch.no_grad():
        out = model(x.to(DEV), t.to(DEV), text_states=ts.to(BF).to(DEV), text_mask=tm.to(DEV), text_states_2=ts2.to(DEV),
                    freqs_cos=cos.to(DEV), freqs_sin=sin.to(DEV), guidance=g.to(DEV))["x"].float().cpu()
    assert model._ws.x4 is not None and model._ws.cat4 is not None, "the MXFP4 path did not run"
    P = MX.Mxfp4Prec()
    sd_q = {k: p.float().cpu() for k, p in model.state_dict().items() if p.dtype != torch.uint8}
    for name, layer in model.named_modules():
        if hasattr(layer, "mx_scale"):
            sd_q[name + ".weight"] = P.mx(layer.weight, layer.mx_scale)
    args = (cfg, x, t, E.r(ts), tm, ts2, cos, sin, g)
    ref_q = R.dit_forward(sd_q, *args, P)              # the contract: MXFP4 activations x MXFP4 weights
    ref_b = R.dit_forward(sd_bf16, *args, E)           # no quantisation at all
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print(f"mxfp4 model: kernel vs oracle {rel(out, ref_q):.4f}, kernel vs bf16 {rel(out, ref_b):.4f}, oracle vs bf16 {rel(ref_q, ref_b):.4f}")
    assert rel(out, ref_q) < 3e-2, rel(out, ref_q)
    assert rel(out, ref_b) < 2 * rel(ref_q, ref_b), (rel(out, ref_b), rel(ref_q, ref_b))
