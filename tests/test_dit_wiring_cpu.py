"""CPU: the checks of tests/dit_wiring.py on the REAL host code (modules/models.py, token_refiner.py, attenion.py, layers.py) with
the kernels replaced by the CPU doubles (tests/cpu_kernel_doubles.py): (1) the correct wiring passes every check at every case;
(2) every mutant - a deliberately mis-wired variant of the host code - is rejected by the check named for it, and one that only a
tolerance can see exceeds that tolerance at least 2x here, so that the rounding of the HIP kernels cannot hide it.  No GPU."""
import pytest
import torch

from tests import cpu_kernel_doubles as KD
from tests import dit_wiring as W


@pytest.fixture(scope="module")
def world():
    """the doubles on ops for the length of this module only (the GPU tests of the same session must meet the real kernels)"""
    from hunyuanvideo_efficiency_amd import ops
    mp = pytest.MonkeyPatch()
    for n in KD.NAMES:
        mp.setattr(ops, n, getattr(KD, n), raising=False)
    yield W.Harness("cpu")
    mp.undo()


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


@pytest.mark.parametrize("name", list(W.MUTANTS))
def test_mutant_is_rejected(world, name):
    make, check, case, stage = W.MUTANTS[name]
    h = W.Harness("cpu")                          # its own models and no entry in the ratio report
    model = h.model(case.model_kind if case is not None else "tiny")
    if check.startswith("A"):
        clean = W.run_named_check(h, check, case)
        assert clean[stage] <= 1.0
        with make(model):
            ratios = W.run_named_check(h, check, case)
        print(f"[dit wiring] mutant {name}: {stage} error / tolerance {ratios[stage]:.2f} (correct wiring {clean[stage]:.3f}) at {case.name}")
        assert ratios[stage] >= 2.0, f"{name}: {stage} is only {ratios[stage]:.2f}x the tolerance at {case.name}"
        return
    W.run_named_check(h, check, case)             # the correct wiring passes the very same call
    with make(model):
        with pytest.raises(AssertionError) as e:
            W.run_named_check(h, check, case)
    print(f"[dit wiring] mutant {name}: rejected by {check}: {e.value}")


def test_zz_ratio_report(world):
    assert world.ratios, "run with the case tests"
    print("\n" + W.report(world))
    assert all(v <= 1.0 for v, _ in world.ratios.values())
