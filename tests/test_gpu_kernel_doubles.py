"""GPU: every CPU kernel double against the kernel it replaces, on the same call (tests/double_parity.py: compare_call, CASES, REFUSALS).

The real wrapper runs on the GPU, the double - called from its module, never installed onto ops / vae_ops in this process - on CPU copies
of the same operands.  Compared per case: the set of written cells of every operand and output buffer (pads, guard rows, columns behind
n0, rows behind n_q), the return value (structure, Python scalars, `is out` identity, shape, dtype, strides of what the callee
allocated) and the values by class.  No kernel-versus-double tolerance exists in this file.

Class and check per op (copy / exact: bit equality; bounded: the named check, passed by kernel and double each on its own):

  copy     patchify, unpatchify (no out, out, strided y), copy3d (ops and the sequence-parallel kernel set), copy4d_, broadcast_row_,
           latent_tile (strided fp32 view, cpad > C), transpose_16b, temporal_nearest_up, temporal_linear_up, fp8_dequant (all 256
           codes), quant_rows_fp8 (the double is the oracle's fp8_quant_rows) - arbitrary bit patterns, NaN payloads, signed zeros
  exact    gemm (B1, B2, B3 of gemm_path: bias, n_split with out1 behind an offset, gate with res in place; B3 also allocating, out wider
           than n0, gate out of place, res without a gate, n_split with gate and res; an `a` with leading dimensions), gemm_fp8 (Q), linear_smallm (M = 1 and 4, addend), gemm_f16
           (out_f32, res, explicit n and k), conv3d_causal (plain, up_t, up_hw, both, res, gn_stats), conv3d_upsampled_subpixel (both
           up_t), conv3d_causal_strided (four strides), conv_cout4 (no affine; ldo 8, 16, 3), groupnorm_apply(silu=False),
           temporal_avg_pool (k = 2, 3), euler_step_, masked_mean, softmax_rows on constant rows, the attention census (attn_fwd, also with
           kv_split_workspace=False, attn_partial with 1 and 2 splits, attn_merge; ops and the sequence-parallel set), the attributes of AttnPartials
  bounded  ln_modulate, ln_modulate_fp8      rowwise_bounds.ln_ref / check (fp8: codes and scales = the oracle's of the side's own bf16 rows)
           qknorm_rope_ (in place, scatter)  rowwise_bounds.qknorm_ref / check, ambiguous elements within 2 ulp
           timestep_embedding                rowwise_bounds.timestep_ref / check
           gemm, gemm_fp8 GELU / SiLU        error_bounds.check on the side's plain product y, and activation_bounds.act_ref / check (fp64
                                             reference, ulp + E32 + FLOOR) of the epilogue on that 16-bit y
           linear_smallm silu_in / silu_out  error_bounds.check (silu_in: on bf16(silu64(x)) of tie-free x), activation_bounds.act_ref / check
           masked_mean (random)              rowwise_bounds.masked_mean_ref / error_bounds.check
           groupnorm_affine(_from_stats)     test_gpu_groupnorm_conditioning.affine_error <= AFFINE_TOL (also for conv3d_causal's gn_stats: the
                                             partial rows differ in layout by design, what the fold makes of them is judged)
           groupnorm_apply(silu=True)        rowwise_bounds.gn_apply_ref / check
           conv_cout4 affine + SiLU          conv_bounds.cout4_act / cout4_ref, rowwise_bounds.check
           softmax_rows (random)             rowwise_bounds.softmax_ref / check
           attn_fwd, attn_partial, attn_merge  attention_bounds.AttnRef.check_o / check_partial / merge_ratio (double: rounded_q=False)

Measured on an MI355X, the largest error-to-bound ratio per op as printed by test_zz_ratio_report (kernel / double):
  ops.attn_fwd 0.605 / 0.473      ops.attn_partial 0.579 / 0.461      ops.attn_merge 0.500 / 0.500       sp.attn_fwd 0.380 / 0.413
  sp.attn_partial 0.579 / 0.461   sp.attn_merge 0.500 / 0.500         ops.gemm 0.500 / 0.500             ops.gemm_fp8 0.500 / 0.500
  ops.linear_smallm 0.484 / 0.484 ops.ln_modulate 0.499 / 0.499       ops.ln_modulate_fp8 0.499 / 0.499  ops.masked_mean 0.500 / 0.500
  ops.qknorm_rope_ 0.500 / 0.500  ops.timestep_embedding 0.499 / 0.499  vae_ops.conv_cout4 0.471 / 0.471  vae_ops.softmax_rows 0.499 / 0.499
  vae_ops.groupnorm_apply 0.499 / 0.499   vae_ops.groupnorm_affine 0.002 / 0.002   vae_ops.groupnorm_affine_from_stats 0.001 / 0.001
(ratios of 0.5 are the final rounding's half ulp: kernel and double are then both the correctly rounded fp64 value.)  Every copy and
exact case is bit-equal.  The conversions to bf16 (patchify, fp8_dequant of the two NaN codes) keep a NaN a NaN in the same cell; the
kernel writes 0x7FC0 where torch's conversion writes 0xFFFF, so those cases compare NaNs as NaNs (Case.any_nan) and everything else bit
for bit.

DELIBERATE_DEVIATIONS (double_parity): sp.attn_suggest_splits (2 from 128 keys on, to exercise both slot counts);
ops.attn_fwd:unrounded-q (the attention doubles do not round q' = bf16(q scale log2 e): held to AttnRef(rounded_q=False));
ops.attn_fwd:narrow-view (the doubles assert n_heads * 128 columns in every view, the wrapper does not).
NO_DOUBLE (double_parity): ops.euler_step_f32_, vae_ops.blend_, vae_ops.postprocess.

Refusals: every illegal call of double_parity.REFUSALS (dtype, innermost stride, non-uniform rows, the 16-byte / 8-element stride rule,
the wrappers' own asserts) breaks one rule and is refused by the wrapper before any launch with the exception type
double_parity.REFUSAL_ERRORS names, every operand and guarded output intact; the CPU tier asserts the same calls and types on the doubles."""
import pytest

pytestmark = pytest.mark.gpu

from tests import double_parity as P  # noqa: E402

RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _libs():
    from hunyuanvideo_efficiency_amd import _lib
    _lib.load()


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_kernel_and_double_agree(case):
    k, d = P.compare_call(P.real_fn(case.op), P.double_fn(case.op), case, "cuda", "cpu")
    if case.cls == "bounded":
        old = RATIOS.get(case.op, (0.0, 0.0))
        RATIOS[case.op] = (max(old[0], k), max(old[1], d))
        print(f"{case.id}: error-to-bound ratio kernel {k:.3f}, double {d:.3f}")
        assert max(k, d) <= 1.0


@pytest.mark.parametrize("ref", P.REFUSALS, ids=[r.id for r in P.REFUSALS])
def test_wrapper_refuses_and_writes_nothing(ref):
    P.check_refusal(P.real_fn(ref.op), ref, "cuda")


def test_zz_ratio_report(capsys):
    with capsys.disabled():
        for op in sorted(RATIOS):
            k, d = RATIOS[op]
            print(f"[kernel doubles] {op}: largest error-to-bound ratio {max(k, d):.3f} (kernel {k:.3f}, double {d:.3f})")
