"""GPU: the checks of tests/vae_wiring.py on the HIP path - the VAE tile coder (AutoencoderKLCausal3D._decode_tile / _encode_tile) as a
composition: topology (64, 128, 256, 256) with the 27-tap, sub-pixel (off / exact / fast) and planes / GEMM conv_out forms at latents
(1, 2, 2), (2, 3, 5), (3, 4, 4) and (3, 3, 5) with per-frame attention; decoder t_ops before / after the first and last resnets (nearest
and trilinear, scale 2 and 3, T = 1); the reduced (32, 64, 128, 128) model with its one-channel groups; mid-block pools (k, s) = (2, 2),
(3, 2), (3, 1) at T = 5, 2, 1 on both halves; the encoder's 884 schedule, down-block pools and a downsample_stride override.

A  every recorded kernel launch against its fp64 restatement on its own operands, every composite stage against the oracle stage in the
   fp16-emulated contract at 4 x the oracle-to-oracle distance (floor: 2 fp16 ulps);
B  every statistics hand-off: identity of the producer, the affine against fp64, the own pass on the same tensor, the hand-written site set;
C  the trace against the reference topology;  D  no recorded call without exactly one check.
That each check rejects the mis-wiring it is meant for is shown on the CPU (tests/test_vae_wiring_cpu.py: every mutant).
The measured ratios are in DESIGN.md ("VAE tile coder wiring tests"); test_zz_ratio_report prints them.  Reads only repository files."""
import pytest

pytestmark = pytest.mark.gpu

from tests import vae_wiring as W  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def world():
    return W.Harness(DEV)


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


def test_zz_ratio_report(world):
    missing = [c.name for c in W.CASES if c.name not in world.ran]
    assert not missing, f"D: cases that did not run: {missing} (run with the case tests)"
    print("\n" + W.report(world))
    assert all(v <= 1.0 for v, _ in world.ratios.values())
