"""GPU: the MXFP4 linears with a low-rank bf16 branch (include/hv_mx_lowrank.h) against tests/mx_lowrank_ref.py and tests/mxfp4_ref.py:
(1) the operand map of the rank stages, exactly; (2) the quantise + down-project pass - codes and scales bit for bit, T inside
tests/error_bounds.py's bound for the bf16 MFMA - at the row-band (128), wave (16) and K-chunk edges; (3) the GEMM inside the worst-case
fp64 bound over the extended operands [dequant(A) | T] and [dequant(W) | Up] at every stage count and parity its loop distinguishes,
epilogues against the kernel's own y; (4) the product error the branch removes; (5) a d = 512 model against its low-rank-aware oracle.
Measured figures: README (MXFP4 low-rank branch)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import error_bounds as EB  # noqa: E402
from tests import mx_lowrank_ref as LR  # noqa: E402
from tests import mxfp4_ref as MX  # noqa: E402
from tests.test_gpu_gemm_mx4 import U, _edge_rows  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402

DEV = "cuda"
E = R.Prec(True)
BF = torch.bfloat16


@pytest.fixture(scope="module")
def lr():
    from hunyuanvideo_efficiency_amd import mx_lowrank, _lib
    _lib.torch_ops()
    return mx_lowrank


@pytest.mark.parametrize("R_", [32, 96])
def test_operand_map_exact(lr, R_):
    """test_operand_and_scale_maps_exact's codes and scales plus integer T and Up that differ along m, n and j: |T Up| <= 6 a term, the
    code products as there, every partial sum exact in fp32 (< 2^20 in units of 2^-4) - a wrong chunk, row deal or stage order shows"""
    M, N, K = 300, 264, 1024
    m, n, k, j = torch.arange(M)[:, None], torch.arange(N)[:, None], torch.arange(K)[None, :], torch.arange(R_)[None, :]
    ca, cw = (m * 7 + k * 3 + (k // 32) * 5) % 16, (n * 5 + k * 11 + (k // 64)) % 16
    pack = lambda c: (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)
    blk = torch.arange(K // 32)[None, :]
    sa, sw = (126 + (m * 3 + blk) % 4).to(torch.uint8), (126 + (n + 2 * blk) % 4).to(torch.uint8)
    t, up = ((m * 3 + j * 5 + j // 8) % 7 - 3).float(), ((n * 2 + j * 3 + j // 32) % 5 - 2).float()
    b = ((torch.arange(N) % 7) - 3).float()
    ref = (MX.dequant(pack(ca), sa).double() @ MX.dequant(pack(cw), sw).double().T + t.double() @ up.double().T + b.double()).to(BF)
    got = lr.gemm_mxfp4_lr(pack(ca).to(DEV), sa.to(DEV), pack(cw).to(DEV), sw.to(DEV), t.to(BF).to(DEV), up.to(BF).to(DEV), b.to(BF).to(DEV))
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("R_", [32, 96, 128])
@pytest.mark.parametrize("K", [512, 640, 3072])
def test_quantise_and_down_project(lr, K, R_):
    """input = a column slice of a wider buffer, outputs = slices of zeroed wider buffers whose padding must stay zero"""
    from hunyuanvideo_efficiency_amd import gemm_mx4
    dn = U((R_, K), f"l.dn{R_}.{K}", 1.0).to(BF)
    worst = 0.0
    for M in (1, 16, 17, 128, 129):
        x = _edge_rows(M, K)
        c_ref, s_ref = MX.quant_rows(x)
        wide = torch.zeros(M, K + 264, dtype=BF, device=DEV)
        wide[:, 264:] = x.to(DEV)
        cw, sw = torch.zeros(M, K // 2 + 32, dtype=torch.uint8, device=DEV), torch.zeros(M, K // 32 + 3, dtype=torch.uint8, device=DEV)
        tw = torch.zeros(M, R_ + 16, dtype=BF, device=DEV)
        c, s, t = lr.quant_rows_mxfp4_lr(wide[:, 264:], dn.to(DEV), codes=cw[:, 16:16 + K // 2], scales=sw[:, 1:1 + K // 32], t=tw[:, 8:8 + R_])
        c0, s0 = gemm_mx4.quant_rows_mxfp4(x.to(DEV))
        assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref) and torch.equal(s, s0) and torch.equal(c, c0), M
        worst = max(worst, EB.check(t.cpu(), EB.gemm_ref(x.float(), dn.float()), BF, f"T {M}x{R_}x{K}"))
        assert int(cw[:, :16].max()) == 0 and int(cw[:, 16 + K // 2:].max()) == 0 and int(sw[:, 0].max()) == 0 and \
            int(sw[:, 1 + K // 32:].max()) == 0 and float(tw[:, :8].abs().max()) == 0 and float(tw[:, 8 + R_:].abs().max()) == 0, M
    print(f"quant_rows_mxfp4_lr K={K} R={R_}: T worst error / bound {worst:.3f}")


def _check_gemm(lr, a, w, dn, up, b, M, N, K):
    """the GEMM on the first M rows of a and N rows of w / up, A and T from the kernel's own pass; then the epilogues against the
    oracle's formulas applied to the kernel's own y (tests/test_gpu_gemm_mx4.py's _check_gemm with the branch).  Returns error / bound."""
    from hunyuanvideo_efficiency_amd import gemm_mx4
    a4, a4s, t = lr.quant_rows_mxfp4_lr(a[:M].to(DEV), dn.to(DEV))
    w4, w4s = gemm_mx4.quant_rows_mxfp4(w[:N].to(DEV))
    ud, bd = up[:N].to(DEV), b[:N].to(DEV)
    args = (a4, a4s, w4, w4s, t, ud, bd)
    got = lr.gemm_mxfp4_lr(*args)
    ref = EB.Ref().add(MX.dequant(a4, a4s), MX.dequant(w4, w4s)).add(t.float().cpu(), up[:N].float()).bias(b[:N].float())
    worst = EB.check(got.cpu(), ref, BF, f"gemm_mxfp4_lr {M}x{N}x{K}+{dn.shape[0]}", worst_case=True)
    y = got.float().cpu()
    got = lr.gemm_mxfp4_lr(*args, act=gemm_mx4.ACT_GELU_TANH)
    torch.testing.assert_close(got.float().cpu(), R.gelu_tanh(y, E), rtol=2 ** -7, atol=2e-2)       # (GELU: exp2-based tanh vs torch's)
    gate, res = U((N,), "f.g", 0.5).to(BF), U((M, N), "f.r").to(BF)
    r_dev = res.to(DEV).clone()
    got = lr.gemm_mxfp4_lr(*args, out=r_dev, gate=gate.to(DEV), res=r_dev)
    assert torch.equal(got.float().cpu(), R.gate_residual(res.float()[None], y[None], gate.float()[None], E)[0])
    if N >= 16:
        ns = (N // 2) // 8 * 8                  # column split (linear1's qkv | mlp) with act1 on the second part
        out0, out1 = torch.zeros(M, ns + 64, dtype=BF, device=DEV), torch.zeros(M, N, dtype=BF, device=DEV)
        lr.gemm_mxfp4_lr(*args, out=out0, n_split=ns, out1=out1[:, 8:], act1=gemm_mx4.ACT_GELU_TANH)
        assert torch.equal(out0[:, :ns].float().cpu(), y[:, :ns]) and float(out0[:, ns:].abs().max()) == 0
        torch.testing.assert_close(out1[:, 8:8 + N - ns].float().cpu(), R.gelu_tanh(y[:, ns:], E), rtol=2 ** -7, atol=2e-2)
        assert float(out1[:, :8].abs().max()) == 0
    return worst


@pytest.mark.parametrize("R_", [32, 64, 96, 128])
@pytest.mark.parametrize("K", [512, 640])
def test_gemm_every_stage_count_and_parity(lr, K, R_):
    a, w, b = U((300, K), f"f.a{K}", 1.5).to(BF), U((520, K), f"f.w{K}", 1.0).to(BF), U((520,), "f.b", 0.1).to(BF)
    dn, up = U((R_, K), f"l.dn{R_}.{K}", 0.05).to(BF), U((520, R_), f"l.up{R_}", 1.0).to(BF)
    worst = max(_check_gemm(lr, a, w, dn, up, b, M, N, K) for M in (1, 257, 300) for N in (8, 264, 520))
    print(f"gemm_mxfp4_lr K={K} R={R_}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("K", [3072, 15360])
def test_gemm_production_depth(lr, K):
    a, w, b = U((33, K), f"f.a{K}", 1.5).to(BF), U((72, K), f"f.w{K}", 1.0).to(BF), U((72,), "f.b", 0.1).to(BF)
    dn, up = U((32, K), f"l.dn32.{K}", 0.05).to(BF), U((72, 32), "l.up32", 1.0).to(BF)
    print(f"gemm_mxfp4_lr K={K} R=32: worst error / bound {_check_gemm(lr, a, w, dn, up, b, 33, 72, K):.3f}")


def test_branch_removes_the_dominant_directions(lr):
    """W = Gaussian + 4 x (rank-4 Gaussian), seed 7, R = 32; error = rms of the product over the fp64 product of the unquantised bf16
    operands.  The kernels' figure must equal the restatement's within 1e-3 (fp32 accumulation and the bf16 output rounding add under
    1e-4 in quadrature), and the restatement's must be at most 0.2 of the branch-less error (0.109 on the CPU).  Measured: README."""
    from hunyuanvideo_efficiency_amd import gemm_mx4
    g = torch.Generator().manual_seed(7)
    a, w = torch.randn(64, 512, generator=g), torch.randn(264, 512, generator=g)
    w = w + 4.0 * torch.randn(264, 4, generator=g) @ torch.randn(4, 512, generator=g)
    a, w = a.to(BF), w.to(BF)
    rel = lambda y: float(((y.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())
    ref = a.double() @ w.double().T
    up, dn, res = LR.factorise(w, 32)
    qa = MX.dequant(*MX.quant_rows(a)).double()
    plain = rel(qa @ MX.dequant(*MX.quant_rows(w)).double().T)
    want = rel(qa @ MX.dequant(*MX.quant_rows(res)).double().T + (a.float() @ dn.float().T).to(BF).double() @ up.double().T)
    a4, a4s, t = lr.quant_rows_mxfp4_lr(a.to(DEV), dn.to(DEV))
    got = rel(lr.gemm_mxfp4_lr(a4, a4s, *gemm_mx4.quant_rows_mxfp4(res.to(DEV)), t, up.to(DEV)).cpu())
    print(f"rank-4 + Gaussian weight, R = 32: no branch {plain:.4f}, restatement {want:.4f}, kernels {got:.4f}, ratio {want / plain:.3f}")
    assert abs(got - want) < 1e-3 and want <= 0.2 * plain, (got, want, plain)


def test_model_lowrank_vs_lowrank_aware_oracle():
    """the d = 512 model of tests/test_gpu_gemm_mx4.py packed with lowrank = 32, within that test's 3e-2 of range of the oracle that adds
    the branch; lowrank = 0 is the path without the argument, bit for bit.  Measured on one MI355X: README."""
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.mxfp4_optimization import convert_mxfp4_linear, enable_mxfp4_linears
    from hunyuanvideo_efficiency_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    thw, txt_len, n_valid = (5, 16, 16), 32, 11
    x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, thw, txt_len, n_valid, seed=2)
    cos, sin = get_nd_rotary_pos_embed(cfg.rope_dim_list, [thw[0], thw[1] // 2, thw[2] // 2], theta=256, use_real=True)
    g, t = torch.tensor([6016.0]), torch.tensor([997.093])

    def run(**kw):
        model = build_model(cfg, DEV)
        assert convert_mxfp4_linear(model, **kw) == 8 + 2 * 2 and enable_mxfp4_linears(model) == 3
        with torch.no_grad():
            out = model(x.to(DEV), t.to(DEV), text_states=ts.to(BF).to(DEV), text_mask=tm.to(DEV), text_states_2=ts2.to(DEV),
                        freqs_cos=cos.to(DEV), freqs_sin=sin.to(DEV), guidance=g.to(DEV))["x"].float().cpu()
        return model, out

    model, out = run(lowrank=32)
    assert all(l.mx_lowrank == 32 for l in model.modules() if hasattr(l, "mx_scale")) and model._ws.lr_t is not None
    P = LR.Mxfp4LowrankPrec()
    sd_q = {k: p.float().cpu() for k, p in model.state_dict().items() if p.dtype != torch.uint8}
    for name, layer in model.named_modules():
        if hasattr(layer, "mx_scale"):
            sd_q[name + ".weight"] = P.mx_lr(layer.weight, layer.mx_scale, layer.mx_lr_up, layer.mx_lr_dn)
    ref_q = R.dit_forward(sd_q, cfg, x, t, E.r(ts), tm, ts2, cos, sin, g, P)
    rel = float((out - ref_q).abs().max() / ref_q.abs().max())
    print(f"mxfp4 model, lowrank = 32: kernel vs low-rank-aware oracle {rel:.4f}")
    assert rel < 3e-2, rel
    assert torch.equal(run(lowrank=0)[1], run()[1])
