"""GPU: the rotated MXFP4 quantisers (include/hv_mx_rot.h) against tests/mx_rot_ref.py, the torch restatement of that header: rotated
unit vectors (no rounding: codes and scales follow from popcount), both kernels bit for bit, the error of a product with outlier
channels, and a d = 512 model against its rotation-aware oracle.  Measured figures: README (MXFP4 rotation)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mx_rot_ref as RR  # noqa: E402
from tests import mxfp4_ref as MX  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from oracle import dit_ref as R  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
ROTS = [16, 64, 256]


@pytest.fixture(scope="module")
def rot():
    from hunyuanvideo_efficiency_amd import mx_rot, _lib
    _lib.torch_ops()
    return mx_rot


def _rows(M, K, key):
    """hashed-random bf16 rows, a few channels 30 times the rest; magnitudes stay in the normal fp32 range"""
    x = syn.hashed_uniform((M, K), key, 23) * (2.0 * math.sqrt(3.0))
    x[:, 5::97] *= 30.0
    return x.to(BF)


@pytest.mark.parametrize("R_", ROTS)
def test_unit_vectors_exact(rot, R_):
    """x = c I (K = max(R, 32): a row is whole MX blocks): row i is column i % R of the Sylvester matrix times c 2^-(log2 R / 2) in
    its own group and zero elsewhere.  The block maximum c 2^-h scales to 4.0 = magnitude index 6, so a code is 6, 14 or 0."""
    K, c, h = max(R_, 32), 8.0, (R_.bit_length() - 1) // 2
    i, j = torch.arange(K)[:, None], torch.arange(K)[None, :]
    neg = torch.tensor([[bin((a % R_) & (b % R_)).count("1") & 1 for b in range(K)] for a in range(K)])
    same = i // R_ == j // R_
    code = torch.where(same, 6 + 8 * neg, 0)
    want_c = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)
    want_s = torch.where(same.reshape(K, K // 32, 32).any(-1), 127 + 3 - h - 2, 0).to(torch.uint8)       # c = 2^3: E = 130 - h
    got_c, got_s = rot.quant_rows_mxfp4_rot((c * torch.eye(K)).to(BF).to(DEV), R_)
    assert torch.equal(got_s.cpu(), want_s) and torch.equal(got_c.cpu(), want_c)


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("K", [256, 768, 3072])
@pytest.mark.parametrize("R_", ROTS)
def test_row_quantiser_bit_exact(rot, R_, K, M):
    x = _rows(M, K, f"r.x{M}.{K}")
    c_ref, s_ref = RR.quant_rows(x, R_)
    c, s = rot.quant_rows_mxfp4_rot(x.to(DEV), R_)
    assert torch.equal(s.cpu(), s_ref) and torch.equal(c.cpu(), c_ref)
    wide = torch.zeros(M, K + 264, dtype=BF, device=DEV)                     # padded ldx; outputs are slices of wider buffers
    wide[:, 264:] = x.to(DEV)
    cw, sw = torch.zeros(M, K // 2 + 32, dtype=torch.uint8, device=DEV), torch.zeros(M, K // 32 + 3, dtype=torch.uint8, device=DEV)
    rot.quant_rows_mxfp4_rot(wide[:, 264:], R_, codes=cw[:, 16:16 + K // 2], scales=sw[:, 1:1 + K // 32])
    assert torch.equal(sw[:, 1:1 + K // 32].cpu(), s_ref) and torch.equal(cw[:, 16:16 + K // 2].cpu(), c_ref)
    assert int(cw[:, :16].max()) == 0 and int(cw[:, 16 + K // 2:].max()) == 0 and int(sw[:, 0].max()) == 0 and int(sw[:, 1 + K // 32:].max()) == 0


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("D", [256, 3072, 4096])
@pytest.mark.parametrize("R_", ROTS)
def test_fused_layernorm_bit_exact(rot, R_, D, M):
    """the header promises hv_ln_modulate_bf16's statistics and rounding: the fused kernel equals the two-kernel composition"""
    from hunyuanvideo_efficiency_amd import ops
    x = _rows(M, D, f"r.ln{M}.{D}").to(DEV)
    sh = (syn.hashed_uniform((D,), "r.sh", 23) * 0.5).to(BF).to(DEV)
    sc = (syn.hashed_uniform((D,), "r.sc", 23) * 0.5).to(BF).to(DEV)
    for shift, scale in ((sh, sc), (None, None), (sh, None), (None, sc)):
        c_ref, s_ref = rot.quant_rows_mxfp4_rot(ops.ln_modulate(x, shift, scale), R_)
        c, s = rot.ln_modulate_mxfp4_rot(x, shift, scale, R_)
        assert torch.equal(s, s_ref) and torch.equal(c, c_ref), (shift is not None, scale is not None)


def _rel_rms(y, ref):
    return float(((y.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())


def test_rotation_cuts_the_outlier_error(rot):
    """error = rms of the MXFP4 product over the fp64 product of the unquantised bf16 operands.  The GPU figure must equal the
    restatement's (its quantisers + an fp64 product) within 1e-3: fp32 accumulation and the bf16 output rounding (2^-9 relative) add
    under 1e-4 in quadrature to 0.16.  Measured: README."""
    from hunyuanvideo_efficiency_amd import gemm_mx4
    g = torch.Generator().manual_seed(7)
    a, w = torch.randn(64, 512, generator=g), torch.randn(64, 512, generator=g)
    a[:, torch.randperm(512, generator=g)[:4]] *= 30.0                       # 1 / 128 of the channels
    a, w = a.to(BF), w.to(BF)
    ref = a.double() @ w.double().T
    ad, wd = a.to(DEV), w.to(DEV)
    plain = _rel_rms(gemm_mx4.gemm_mxfp4(*gemm_mx4.quant_rows_mxfp4(ad), *gemm_mx4.quant_rows_mxfp4(wd)).cpu(), ref)
    plain_ref = _rel_rms(MX.dequant(*MX.quant_rows(a)).double() @ MX.dequant(*MX.quant_rows(w)).double().T, ref)
    print(f"no rotation: kernel {plain:.4f}, restatement {plain_ref:.4f}")
    assert abs(plain - plain_ref) < 1e-3
    for R_ in ROTS:
        got = _rel_rms(gemm_mx4.gemm_mxfp4(*rot.quant_rows_mxfp4_rot(ad, R_), *rot.quant_rows_mxfp4_rot(wd, R_)).cpu(), ref)
        want = _rel_rms(MX.dequant(*RR.quant_rows(a, R_)).double() @ MX.dequant(*RR.quant_rows(w, R_)).double().T, ref)
        print(f"R = {R_}: kernel {got:.4f}, restatement {want:.4f}, ratio to no rotation {got / plain:.3f}")
        assert abs(got - want) < 1e-3 and got <= 0.9 * plain, (R_, got, want, plain)


def test_model_rotated_vs_rotation_aware_oracle():
    """the d = 512 model of tests/test_gpu_gemm_mx4.py packed with rot = 64, within that test's 3e-2 of range of the oracle that rotates
    both operands; rot = 0 is the path without the argument, bit for bit.  Measured on one MI355X: README."""
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

    model, out = run(rot=64)
    assert all(l.mx_rot == 64 for l in model.modules() if hasattr(l, "mx_scale"))
    P = RR.Mxfp4RotPrec(64)
    sd_q = {k: p.float().cpu() for k, p in model.state_dict().items() if p.dtype != torch.uint8}
    for name, layer in model.named_modules():
        if hasattr(layer, "mx_scale"):
            sd_q[name + ".weight"] = P.mx(layer.weight, layer.mx_scale)
    ref_q = R.dit_forward(sd_q, cfg, x, t, R.Prec(True).r(ts), tm, ts2, cos, sin, g, P)
    rel = float((out - ref_q).abs().max() / ref_q.abs().max())
    print(f"mxfp4 model, rot = 64: kernel vs rotation-aware oracle {rel:.4f}")
    assert rel < 3e-2, rel
    assert torch.equal(run(rot=0)[1], run()[1])
