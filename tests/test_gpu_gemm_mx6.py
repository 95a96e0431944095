"""GPU: the opt-in MXFP6 linears (include/hv_gemm_mx6.h) against tests/mxfp6_ref.py, the torch restatement of that header.

(1) operand and scale maps of v_mfma_scale_f32_16x16x128_f8f6f4 with 6-register FP6 operands as the kernel feeds it: exactly
representable data, every partial sum exact in fp32, so the output is the bf16 rounding of the fp64 product, bit for bit - this is the
test that decides the header's packing rule; (2) both quantisers bit for bit; (3) the GEMM on random data given the same quantised
operands, element by element inside tests/error_bounds.py's worst-case form, at every K-stage count the loop distinguishes - K / 128 = 4
(the minimum: the tail alone) .. 7 (one past ring depth 3 x unroll 2, with and without the peeled front iteration) - and at K = 15360;
(4) a d = 512 model against the quantisation-aware oracle.  Measured figures: README (MXFP6 linears)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import error_bounds as EB  # noqa: E402
from tests import mxfp4_ref as MX4  # noqa: E402
from tests import mxfp6_ref as MX  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402

DEV = "cuda"
E = R.Prec(True)
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    """the MXFP6 wrappers (hunyuanvideo_efficiency_amd.gemm_mx6, with the activation constants of ops)"""
    from hunyuanvideo_efficiency_amd import gemm_mx6, _lib
    _lib.torch_ops()
    return gemm_mx6


def U(shape, key, scale=1.0):
    return syn.hashed_uniform(shape, key, 23) * (scale * math.sqrt(3.0))


def test_operand_and_scale_maps_exact(ops):
    """All 64 codes, and scales that differ along m, n, k and per (row, block): a wrong bit order inside the 24 bytes, a k-block or row
    from the wrong place, or a wrong op_sel byte (A: rows 16, 32, 48 away; W, dealt by w_tile_row: rows 4, 32, 36 away) changes the
    result.  e2m3 values are multiples of 1/8 and the scales are 2^-1 .. 2^2, so every product is a multiple of 2^-8; the test asserts
    that sum |a| |w| + |bias| stays below 2^24 of these units for every output, which bounds every partial sum in any order: fp32
    accumulation is exact."""
    M, N, K = 300, 264, 1024
    m, n, k = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :]
    ca, cw = (m * 7 + (m // 16) * 5 + k * 3 + (k // 32) * 5) % 64, (n * 5 + (n // 4) * 3 + k * 11 + (k // 64)) % 64
    blk = torch.arange(K // 32)[None, :]
    sa = (126 + (m // 16 + m + blk) % 4).to(torch.uint8)
    sw = (126 + (n // 4 + (n // 32) * 2 + blk // 2) % 4).to(torch.uint8)
    b = ((torch.arange(N) % 7) - 3).float()
    qa, qw = MX.pack(ca), MX.pack(cw)
    A, W = MX.dequant(qa, sa).double(), MX.dequant(qw, sw).double()
    assert float((A.abs() @ W.abs().T).max() + 3) * 2 ** 8 < 2 ** 24
    ref = (A @ W.T + b.double()).to(BF)
    got = ops.gemm_mxfp6(qa.to(DEV), sa.to(DEV), qw.to(DEV), sw.to(DEV), b.to(BF).to(DEV))
    assert torch.equal(got.cpu(), ref)


def _edge_rows(M, K):
    """random rows whose first blocks are the contract's edge cases: zero; maximum a power of two; maximum just below one (saturates at
    7.5); ties at every midpoint of the 32 magnitudes times the scale, both signs (two blocks); subnormals only"""
    x = U((M, K), f"q.x{M}.{K}", 2.0).to(BF)
    x[:, 0:32] = 0
    x[:, 32:64] = (U((M, 32), "q.p2", 1.0).clamp(-3.9, 3.9)).to(BF)
    x[:, 40] = 4.0
    x[:, 64:96] = x[:, 32:64]
    x[:, 72] = -3.984375
    ties = torch.tensor([mid for mid, _ in MX.MID] + [7.5]) * 2.0 ** -3          # 31 midpoints (at most 8 significant bits: bf16) + the maximum
    x[:, 96:128] = ties.to(BF)
    x[:, 128:160] = -ties.to(BF)
    sub = ((torch.arange(32) * 4 + 1) % 128).to(torch.int16)
    sub[1::2] |= -32768
    x[:, 160:192] = sub.view(BF)
    return x


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("K", [512, 2560])
def test_quantisers_bit_exact(ops, M, K):
    x = _edge_rows(M, K)
    assert torch.equal(x[:, 96:128].float(), torch.tensor([mid for mid, _ in MX.MID] + [7.5]).expand(M, 32) / 8)      # the ties survived bf16
    c_ref, s_ref = MX.quant_rows(x)
    c, s = ops.quant_rows_mxfp6(x.to(DEV))
    assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref)
    assert int(s_ref[0, 0]) == 0 and int(c_ref[0, :24].max()) == 0 and int(s_ref[0, 5]) == 0 and int(c_ref[0, 120:144].max()) > 0
    assert int(MX.unpack(c_ref)[0, 72]) == 63 and MX.unpack(c_ref)[0, 96:128].tolist() == [(i + 1) // 2 * 2 for i in range(31)] + [31]
    wide = torch.zeros(M, K + 512, dtype=BF, device=DEV)          # strided input: a column slice of a wider buffer, as cat[:, d:]
    wide[:, 512:] = x.to(DEV)
    c, s = ops.quant_rows_mxfp6(wide[:, 512:])
    assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref)
    # fused LayerNorm: the kernel's statistics are fp32 sums in its own order, so its bf16 LayerNorm output may sit one ulp from the
    # restatement's on a few elements, and only there may a code differ.  CAP (the project's cap, on unpacked codes) bounds that
    # share; the restatement itself, run in two summation orders (fp32 and fp64 statistics), must stay inside it on these inputs.
    CAP = 0.02
    xr = U((M, K), f"q.ln{M}.{K}", 2.0).to(BF)
    sh, sc = U((K,), "q.sh", 0.3).to(BF), U((K,), "q.sc", 0.3).to(BF)
    y = E.r(R.ln_modulate(xr.float()[None], sh.float()[None], sc.float()[None], E))[0]
    x64 = xr.double()
    n64 = (x64 - x64.mean(-1, keepdim=True)) / (x64.var(-1, unbiased=False, keepdim=True) + 1e-6).sqrt()
    y64 = E.r((n64.float() * E.r(1.0 + sc.float()) + sh.float()))
    c_ref, s_ref = MX.quant_rows(y)
    assert float((MX.unpack(MX.quant_rows(y64)[0]) != MX.unpack(c_ref)).float().mean()) < CAP
    c, s = ops.ln_modulate_mxfp6(xr.to(DEV), sh.to(DEV), sc.to(DEV))
    assert torch.equal(s.cpu(), s_ref)
    share = float((MX.unpack(c) != MX.unpack(c_ref)).float().mean())
    print(f"ln_modulate_mxfp6 M={M} K={K}: share of codes that differ {share:.4f}")
    assert share < CAP


WORST = {}


def _check_gemm(ops, a, w, b, M, N, K):
    """the kernel on the first M rows of a and N rows of w, quantised by the kernel's own quantiser, against fp64 over the dequantised
    operands; then the epilogues, exactly, against the oracle's formulas applied to the kernel's own y"""
    a6, a6s = ops.quant_rows_mxfp6(a[:M].to(DEV))
    w6, w6s = ops.quant_rows_mxfp6(w[:N].to(DEV))
    bd = b[:N].to(DEV)
    got = ops.gemm_mxfp6(a6, a6s, w6, w6s, bd)
    ref = EB.gemm_ref(MX.dequant(a6, a6s), MX.dequant(w6, w6s), b[:N].float())
    WORST[K] = max(WORST.get(K, 0.0), EB.check(got.cpu(), ref, BF, f"gemm_mxfp6 {M}x{N}x{K}", worst_case=True))
    y = got.float().cpu()
    got = ops.gemm_mxfp6(a6, a6s, w6, w6s, bd, act=ops.ACT_GELU_TANH)
    torch.testing.assert_close(got.float().cpu(), R.gelu_tanh(y, E), rtol=2 ** -7, atol=2e-2)       # (GELU: exp2-based tanh vs torch's)
    gate, res = U((N,), "f.g", 0.5).to(BF), U((M, N), "f.r").to(BF)
    r_dev = res.to(DEV).clone()
    got = ops.gemm_mxfp6(a6, a6s, w6, w6s, bd, out=r_dev, gate=gate.to(DEV), res=r_dev)
    assert torch.equal(got.float().cpu(), R.gate_residual(res.float()[None], y[None], gate.float()[None], E)[0])
    if N >= 16:
        ns = (N // 2) // 8 * 8                  # column split (linear1's qkv | mlp) with act1 on the second part
        out0 = torch.zeros(M, ns + 64, dtype=BF, device=DEV)
        out1 = torch.zeros(M, N, dtype=BF, device=DEV)
        ops.gemm_mxfp6(a6, a6s, w6, w6s, bd, out=out0, n_split=ns, out1=out1[:, 8:], act1=ops.ACT_GELU_TANH)
        assert torch.equal(out0[:, :ns].float().cpu(), y[:, :ns]) and float(out0[:, ns:].abs().max()) == 0
        torch.testing.assert_close(out1[:, 8:8 + N - ns].float().cpu(), R.gelu_tanh(y[:, ns:], E), rtol=2 ** -7, atol=2e-2)
        assert float(out1[:, :8].abs().max()) == 0


@pytest.mark.parametrize("K", [512, 640, 768, 896])
def test_gemm_random_same_operands(ops, K):
    a, w, b = U((300, K), f"f.a{K}", 1.5).to(BF), U((520, K), f"f.w{K}", 1.0).to(BF), U((520,), "f.b", 0.1).to(BF)
    for M in (1, 257, 300):
        for N in (8, 264, 520):
            _check_gemm(ops, a, w, b, M, N, K)
    print(f"gemm_mxfp6 K={K}: worst error / bound {WORST[K]:.3f}")


def test_gemm_production_depth(ops):
    K = 15360
    a, w, b = U((33, K), "f.a15", 1.5).to(BF), U((72, K), "f.w15", 1.0).to(BF), U((72,), "f.b", 0.1).to(BF)
    _check_gemm(ops, a, w, b, 33, 72, K)
    print(f"gemm_mxfp6 K={K}: worst error / bound {WORST[K]:.3f}")


def test_model_mxfp6_vs_quantisation_aware_oracle():
    """Measured on one MI355X: see README (MXFP6 linears)."""
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.mxfp6_optimization import convert_mxfp6_linear, enable_mxfp6_linears
    from hunyuanvideo_efficiency_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    model = build_model(cfg, DEV)
    sd_bf16 = {k: p.float().cpu() for k, p in model.state_dict().items()}
    assert convert_mxfp6_linear(model) == 8 + 2 * 2 and enable_mxfp6_linears(model) == 3
    with pytest.raises(RuntimeError, match="mxfp6"):
        model.single_blocks[0].linear1.w()
    thw, txt_len, n_valid = (5, 16, 16), 32, 11
    x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, thw, txt_len, n_valid, seed=2)
    T, H, W = thw
    cos, sin = get_nd_rotary_pos_embed(cfg.rope_dim_list, [T, H // 2, W // 2], theta=256, use_real=True)
    g, t = torch.tensor([6016.0]), torch.tensor([997.093])
    with torch.no_grad():
        out = model(x.to(DEV), t.to(DEV), text_states=ts.to(BF).to(DEV), text_mask=tm.to(DEV), text_states_2=ts2.to(DEV),
                    freqs_cos=cos.to(DEV), freqs_sin=sin.to(DEV), guidance=g.to(DEV))["x"].float().cpu()
    assert model._ws.x6 is not None and model._ws.cat6 is not None and model._ws.x4 is None, "the MXFP6 path did not run"
    P, P4 = MX.Mxfp6Prec(), MX4.Mxfp4Prec()
    sd_q = {k: p.float().cpu() for k, p in model.state_dict().items() if p.dtype != torch.uint8}
    sd_4 = dict(sd_bf16)
    for name, layer in model.named_modules():
        if hasattr(layer, "mx_scale"):
            sd_q[name + ".weight"] = P.mx(layer.weight, layer.mx_scale)
            sd_4[name + ".weight"] = P4.mx(*MX4.quant_rows(E.r(sd_bf16[name + ".weight"])))
    args = (cfg, x, t, E.r(ts), tm, ts2, cos, sin, g)
    ref_q = R.dit_forward(sd_q, *args, P)              # the contract: MXFP6 activations x MXFP6 weights
    ref_4 = R.dit_forward(sd_4, *args, P4)             # the same model under the MXFP4 restatement
    ref_b = R.dit_forward(sd_bf16, *args, E)           # no quantisation at all
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print(f"mxfp6 model: kernel vs oracle {rel(out, ref_q):.4f}, kernel vs bf16 {rel(out, ref_b):.4f}, oracle vs bf16 {rel(ref_q, ref_b):.4f}, "
          f"mxfp4 oracle vs bf16 {rel(ref_4, ref_b):.4f}")
    assert rel(out, ref_q) < 3e-2, rel(out, ref_q)
    assert rel(out, ref_b) < 2 * rel(ref_q, ref_b), (rel(out, ref_b), rel(ref_q, ref_b))
    assert rel(ref_q, ref_b) < 0.5 * rel(ref_4, ref_b), (rel(ref_q, ref_b), rel(ref_4, ref_b))
