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


def test_zz_ratio_report(world):
    assert world.ratios, "run with the case tests"
    print("\n" + W.report(world))
    assert all(v <= 1.0 for v, _ in world.ratios.values())
