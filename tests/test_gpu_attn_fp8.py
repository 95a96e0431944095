"""GPU: the opt-in FP8 attention of include/hv_attn_fp8.h.

(1) The quantiser, bit for bit: means, scales and e4m3 bytes of the workspace equal a torch restatement in fp32 in the header's order
(`restate`), after the header's V permutation and transposition are undone (`unpack`); both live in tests/attn_fp8_ref.py, which the
CPU doubles share.

(2) The kernel against fp64 attention over the DEQUANTISED operands (sq Q8, sk K8, sv V8, log2 domain), element by element.  With w_j
the fp64 softmax weights, l = sum_j 2^(s_j - M) >= 1 and v~ the dequantised V, the bound per output element d is (attn_fp8_ref.fp8_bound)

    ulp_bf16(O64_d)                                                   the final rounding (EB.ulp_out)
  + sum_j max(2^-4 w_j, 2^-18 / l) |v~_jd|                            e4m3(p 2^8): half an ulp relative (3 mantissa bits) down to
                                                                      p 2^8 = 2^-6, half the subnormal spacing 2^-10 below; a p rounded
                                                                      against an earlier, smaller running maximum is scaled down after
  + sum_j eta_j w_j |v~_jd - O64_d|,  eta_j = ln 2 bs_j + 2^-22        a relative error of p_j shared by numerator and row sum (the form of
                                                                      attention_bounds.py); bs_j = C sqrt(128) 2^-24 S_j + 2^-22 (|s_j| +
                                                                      |M|): the 128-term reduction of the fp8 MFMA in the worst-case form
                                                                      error_bounds.py prescribes for it (S_j = sum_c |q'_c k_jc|), then the
                                                                      two scale multiplies and the subtraction of m; 2^-22 for v_exp_f32
  + C sqrt(n_kv) 2^-24 (sum_j w_j |v~_jd| + 2 |O64_d|)                fp32 accumulation of P.V and l, the per-tile rescales and the epilogue,
                                                                      worst-case form as well.
No term is fitted to the kernel.  `peaked` pins the V permutation and the operand lane maps (one key owns the row: another key's v is far
outside 2^-4 |v|), `phantom` the tail mask, `flat` P = 1 everywhere.

(3) The tiny model with enable_fp8_attention against itself without: different bytes (the path is taken) within 1e-1 of the output range,
the figure tests/test_gpu_fp8_mfma.py uses for an FP8 approximation against non-FP8 semantics; the flag with an SP object raises."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import attention_bounds as AB  # noqa: E402
from tests.attn_fp8_ref import dequantised, fp8_bound, restate, unpack  # noqa: E402

DEV = "cuda"
FP8 = torch.float8_e4m3fn
D, KVT = 128, 64


@pytest.fixture(scope="module")
def ops():
    from hunyuanvideo_efficiency_amd import ops as _ops, _lib
    _lib.torch_ops()
    return _ops


def fused(q, k, v, H):
    """q, k, v as views into one fused [n, 3 H 128] buffer (n_q and n_kv differ: the longer one sets the rows)"""
    buf = torch.zeros(max(q.shape[0], k.shape[0]), 3 * H * D, dtype=torch.bfloat16, device=DEV)
    buf[:q.shape[0], :H * D], buf[:k.shape[0], H * D:2 * H * D], buf[:k.shape[0], 2 * H * D:] = q.to(DEV), k.to(DEV), v.to(DEV)
    return buf[:q.shape[0], :H * D], buf[:k.shape[0], H * D:2 * H * D], buf[:k.shape[0], 2 * H * D:]


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n_kv", [1, 63, 64, 65, 129])
def test_quantiser_bit_exact(ops, n_kv, H):
    n_q = 5
    q, k, v = AB.make_case("random", n_q, n_kv, H, f"q8.{n_kv}.{H}")
    q[0] = 0                                            # an all-zero row: scale 1, codes 0
    q[1] = (q[1].float() * 2.0 ** -120).to(q.dtype)     # amax below 448 * 2^-126: the scale floor
    v[:, 5] = 0                                         # an all-zero channel of V
    ws = ops.attn_fp8_quantise(*fused(q, k, v, H), H)
    got, want = unpack(ws, n_q, n_kv, H), restate(q, k, v, H, ops.ATTN_FP8["HV_ATTN_FP8_STAT_KEYS"])
    assert float(want["sq"][0, 0]) == 1.0 and float(want["sq"][1, 0]) == 2.0 ** -126 and float(want["sv"][0, 5]) == 1.0
    for name, w in want.items():
        g = got[name].cpu()
        same = torch.equal(g.view(torch.uint8), w.contiguous().view(torch.uint8)) if w.dtype == FP8 else torch.equal(g, w)
        assert same, f"{name} differs from the restatement (n_kv {n_kv}, {H} heads)"


BM, RING = 256, 3


@pytest.mark.parametrize("cls", AB.CLASSES)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("n_kv", [1, 63, 64, 65, KVT * RING - 1, KVT * RING + 1, KVT * (RING + 2) + 5])
@pytest.mark.parametrize("n_q", [1, 31, 33, BM + 1])
def test_kernel_within_fp64_bound(ops, n_q, n_kv, H, cls):
    assert (BM, RING) == (ops.ATTN_FP8["HV_ATTN_FP8_BM"], ops.ATTN_FP8["HV_ATTN_FP8_RING"])
    q, k, v = fused(*AB.make_case(cls, n_q, n_kv, H, f"f8.{n_q}.{n_kv}.{H}"), H)
    out = torch.full((n_q, H * D + 64), 7.0, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(ops.attn_fp8_workspace_bytes(n_q, n_kv, H) + 512, dtype=torch.uint8, device=DEV)
    ops.attn_fwd_fp8(q, k, v, out[:, :H * D], H, workspace=ws)
    assert bool((out[:, H * D:] == 7.0).all()), "guard columns behind the output were written"
    u = unpack(ws, n_q, n_kv, H)
    worst = 0.0
    for h in range(H):
        O, bound = fp8_bound(*dequantised(u, h, n_kv), n_kv)
        got = out[:, h * D:(h + 1) * D].double()
        assert bool(torch.isfinite(got).all())
        ratio = (got - O).abs() / bound
        worst = max(worst, float(ratio.max()))
        i, d = divmod(int(ratio.argmax()), D)
        assert float(ratio.max()) <= 1.0, (f"{cls} n_q {n_q} n_kv {n_kv} head {h}/{H}: {int((ratio > 1).sum())} elements outside the bound, worst "
                                           f"{float(ratio.max()):.3g} at row {i} dim {d}: got {float(got[i, d])}, O64 {float(O[i, d]):.6g}")
    print(f"fp8 attention {cls} {n_q}x{n_kv}x{H}: worst error / bound {worst:.3f}")


def _tiny_model_run(model, cfg):
    from hunyuanvideo_efficiency_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    thw, txt_len, n_valid = (5, 16, 16), 32, 11
    x, ts, tm, ts2 = syn.synth_dit_inputs(cfg, thw, txt_len, n_valid, seed=2)
    cos, sin = get_nd_rotary_pos_embed(cfg.rope_dim_list, [thw[0], thw[1] // 2, thw[2] // 2], theta=256, use_real=True)
    with torch.no_grad():
        return model(x.to(DEV), torch.tensor([997.093]).to(DEV), text_states=ts.to(torch.bfloat16).to(DEV), text_mask=tm.to(DEV),
                     text_states_2=ts2.to(DEV), freqs_cos=cos.to(DEV), freqs_sin=sin.to(DEV),
                     guidance=torch.tensor([6016.0]).to(DEV))["x"].float().cpu()


def test_model_with_fp8_attention(ops):
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.modules.fp8_optimization import enable_fp8_attention
    cfg = syn.DiTConfig(hidden_size=512, heads_num=4, mm_double_blocks_depth=1, mm_single_blocks_depth=2)
    model = build_model(cfg, DEV)
    off = _tiny_model_run(model, cfg)
    assert model._ws.attn8 is None and enable_fp8_attention(model) == 3
    on = _tiny_model_run(model, cfg)
    assert model._ws.attn8 is not None and not torch.equal(on, off), "the FP8 attention path did not run"
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    print(f"fp8 attention, tiny model: {rel(on, off):.4g} of the output range")
    assert rel(on, off) < 1e-1 and rel(off, on) < 1e-1, (rel(on, off), rel(off, on))
    assert enable_fp8_attention(model, False) == 3 and torch.equal(_tiny_model_run(model, cfg), off)
    # the flag together with a sequence-parallel object: an error that names both, never a silent bf16 run
    enable_fp8_attention(model)
    for block in list(model.double_blocks) + list(model.single_blocks):
        block.hybrid_seq_parallel_attn = object()
    with pytest.raises(NotImplementedError, match="fp8_attention.*hybrid_seq_parallel_attn"):
        _tiny_model_run(model, cfg)
