"""GPU: the checks of tests/dit_wiring.py on the HIP path - the DiT forward as a composition, at the text-mask and token-count edges
(s_img 1, 45, 64, 320, 255, 257; (s_txt, n_valid) (32,0) (32,1) (32,11) (32,31) (32,32) (1,1) (1,0) (9,4) (256,77); text_mask=None,
use_attention_mask=False, no RoPE tables, no guidance embedding; the FP8-MFMA configuration on four of them).

A  every stage (dit_vec, patch_embed, token_refiner, double_block, single_block, final_layer + unpatchify) on the GPU's own input
   against the oracle stage in Prec(True), at the block tolerance of test_gpu_model.py::test_block_call_surfaces_vs_oracle (rtol 2^-6,
   atol 6e-2); the block call surfaces with a wide vec at the same tolerance; the whole output at 3e-2 of its range.
B  bitwise: padding text content, both sides of cu1, the RoPE table edge, repeat, re-key, refiner cache, batch rows.
That each check rejects the mis-wiring it is meant for is shown on the CPU (tests/test_dit_wiring_cpu.py: every mutant, and at
least 2x the tolerance where only a tolerance sees it).

MI355X, largest error / tolerance over all cases (test_zz_ratio_report prints them):
  dit_vec 0.008, patch_embed 0.000, token_refiner 0.111, double_block img 0.198 / txt 0.202, single_block 0.170,
  final_layer + unpatchify 0.056; block call surfaces (vec half-width 1.5): double img 0.206 / txt 0.205, single 0.169;
  whole output 6.6e-3 of range (0.22 of 3e-2), FP8-MFMA configuration 7.4e-3 (0.25).

Segment level (dit_wiring.check_segment_attention): attenion.segment_attention_ under tile_plan and under fp8_attention on a qkv buffer
made by the test, s_img 1, 45, 320 x n_valid 0, 1, s_txt = 32.  Every output row against the fp64 reference of its own key set (image
rows: the window restated by attn_tile_plans.allowed plus [s_img, cu1); valid-text rows: [0, cu1); padding rows: [cu1, S); AttnRef's
bound, under FP8 attn_fp8_ref.fp8_bound over the workspace the call filled), then B8 bitwise: k / v of row cu1 leave rows [0, cu1)
bit-equal and change the padding rows, row cu1 - 1 changes image rows, one image token changes exactly the tiles whose window holds it
and every valid-text row.  MI355X, worst error / bound: tile_plan 0.523, fp8_attention 0.709 (s_img 1, n_valid 1).

Model level under the opt-in flags (dit_wiring.STA_CASES, FP8ATTN_CASES; the tiny config).  enable_sliding_tile_attention: A against the
WINDOWED oracle (oracle.dit_ref.attention_varlen replaced for segment 1 by R.sdpa with the mask attn_tile_plans.allowed restates, plus
the valid text; text queries see all of [0, cu1)) at the block tolerance, the whole output at 3e-2 of range, B1, B3, B4; re-keying
between two grids; a grid change at equal s_img (latent (2, 8, 16), (4, 8, 8), the first again: the second run has the bits of a fresh
model, the third those of the first); batch rows; block.forward without a plan raises.  enable_fp8_attention: the whole output within
1e-1 of the range of the unflagged oracle, B1, B4, re-keying larger -> smaller -> larger (the grow-only workspace reused), batch rows.
MI355X: under the window no stage above the figures of the first paragraph (double_block img 0.198), whole output 6.6e-3 of range (0.22 of
3e-2, one tile of one chunk, n_valid 1); under FP8 attention whole output 6.6e-3 of range (0.066 of 1e-1).
The mutants (dit_wiring.MUTANTS: dense=(s_img, S), dense=(s_img + 1, cu1), text queries not launched, the plan of the previous grid
reused, FP8 over [0, S), cu1 +- 1 under either flag) patch the ops call sites, models.model_plan or models.segment_attention_, and
are rejected on the CPU tier only (tests/test_dit_wiring_cpu.py).
"""
import pytest

pytestmark = pytest.mark.gpu

from tests import dit_wiring as W  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def world():
    return W.Harness(DEV)


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_case_passes_stage_and_exact_checks(world, case):
    W.check_case(world, case)


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_block_call_surfaces_both_sides_of_cu1(world, case):
    W.check_block_call_surfaces(world, world.model(case.model_kind), case)


def test_text_mask_none_is_an_all_ones_mask(world):
    W.check_mask_none_equals_ones(world)


@pytest.mark.parametrize("b", [W.Case((5, 16, 16), 256, 77), W.Case((1, 2, 2), 9, 4)], ids=["B-larger", "B-smaller"])
def test_rekey_a_b_a(world, b):
    W.check_rekey(world, world.model("tiny"), W.Case((3, 6, 10), 32, 11), b)


def test_refiner_cache_follows_in_place_edits(world):
    W.check_cache(world)


def test_batch_rows_equal_single_sample_runs(world):
    W.check_batch(world)


@pytest.mark.parametrize("i", range(len(W.FP8_CASES)), ids=[c.name for c in W.FP8_CASES])
def test_fp8_mfma_configuration(world, i):
    W.check_fp8_case(world, W.FP8_CASES[i], W.FP8_CASES[(i + 1) % len(W.FP8_CASES)])


@pytest.mark.parametrize("case", W.STA_CASES + W.FP8ATTN_CASES, ids=lambda c: c.name)
def test_opt_in_attention_case(world, case):
    W.check_flag_case(world, case)


def test_sliding_tile_plan_follows_a_grid_change_at_equal_s_img(world):
    W.check_grid_change(world)


def test_block_forward_without_a_plan_raises(world):
    W.check_no_plan_raises(world)


@pytest.mark.parametrize("flag", ["sta", "fp8attn"])
def test_rekey_under_the_opt_in_flags(world, flag):
    W.check_flag_rekey(world, flag)


@pytest.mark.parametrize("flag", ["sta", "fp8attn"])
def test_batch_rows_under_the_opt_in_flags(world, flag):
    W.flag_model(world, W.STA_CASES[0] if flag == "sta" else W.FP8ATTN_CASES[0])
    W.check_batch(world, flag)


SEGMENT_RATIOS = {}


@pytest.mark.parametrize("n_valid", [0, 1, W.SEGMENT_S_TXT])
@pytest.mark.parametrize("s_img", sorted(W.SEGMENT_GEOS))
@pytest.mark.parametrize("flag", ["sta", "fp8attn"])
def test_segment_attention_under_the_opt_in_flags(flag, s_img, n_valid):
    r = W.check_segment_attention(DEV, flag, s_img, n_valid)
    SEGMENT_RATIOS[flag] = max(SEGMENT_RATIOS.get(flag, 0.0), r)
    print(f"[dit wiring] segment attention {flag} s_img {s_img} n_valid {n_valid}: worst error / bound {r:.3f}")


def test_zz_ratio_report(world):
    assert world.ratios, "run with the case tests"
    print("\n" + W.report(world))
    for flag, r in sorted(SEGMENT_RATIOS.items()):
        print(f"[dit wiring]   segment attention under {flag:<8s} {r:.3f}  (worst error / fp64 bound)")
    assert all(v <= 1.0 for v, _ in world.ratios.values())
