"""CPU: the checks of tests/vae_wiring.py on the REAL host code of the VAE tile coder (AutoencoderKLCausal3D._decode_tile, _encode_tile,
_mid_block, _resnet, _mid_attention, _conv, _gn, _prepare) with the kernels replaced by the CPU doubles (tests/cpu_kernel_doubles.py):
(1) the correct wiring passes A, B, C and D at every case; (2) every mutant - a deliberately mis-wired variant of the host code - is
rejected, and the assertion message names the check that rejected it.  No GPU."""
import pytest

from tests import cpu_kernel_doubles as KD
from tests import vae_wiring as W


@pytest.fixture(scope="module")
def world():
    """the doubles on vae_ops for the length of this module only (the GPU tests of the same session must meet the real kernels)"""
    mp = pytest.MonkeyPatch()
    KD.install_vae_tile_coder(mp)
    yield W.Harness("cpu")
    mp.undo()


@pytest.mark.parametrize("case", W.CASES, ids=lambda c: c.name)
def test_case_passes_every_check(world, case):
    W.check_case(world, case)


@pytest.mark.parametrize("name", ["A-2x3x5-fast-planes", "B-3x4x4"])
def test_handoff_disabled_is_the_same_function(world, name):
    case = W.CASE[name]
    out, thw, rec = world.run(case)
    W.check_handoff_disabled(world, case, out, rec)


def test_second_call_after_clearing_t_ops(world):
    W.check_second_call(world, W.CASE["A-tops-both"])


@pytest.mark.parametrize("name", list(W.MUTANTS))
def test_mutant_is_rejected(world, name):
    h = W.Harness("cpu")                          # no entry in the ratio report
    h._models, h._sd = world._models, world._sd   # the prepared models are shared; a mutant patches and restores
    msg = W.run_mutant(h, name)
    print(f"[vae wiring] mutant {name}: rejected by check {msg[:1]}: {msg[:300]}")


def test_zz_ratio_report(world):
    missing = [c.name for c in W.CASES if c.name not in world.ran]
    assert not missing, f"D: cases that did not run: {missing} (run with the case tests)"
    print("\n" + W.report(world))
    assert all(v <= 1.0 for v, _ in world.ratios.values())
