"""GPU, 2 / 3 / 4 / 8 ranks sharing the ONE card of the test box: the checks of tests/sp_wiring.py on the HIP kernels.  RCCL refuses two
ranks on one device, so the collectives are staged through the host and carried by gloo (tests/sp_gpu_helpers.py) - a test-only
transport; every byte of compute is the product's kernels.

Part 1 (test_attention_object_equals_single_rank_replay): UlyssesLongContextAttention through __call__, run_fused and begin / send or
send_packed / attend_async, at every geometry of sp_wiring.GEOS, against a single-rank replay - bit for bit (A1), the replay against the
fp64 bound of tests/attention_bounds.py (A2), and for the rings a key census (A3).  Part 2 (test_sharded_model_stage_by_stage): the
sharded d = 512 model traced on every rank - every block against the oracle on its own gathered input (B1), the replicated text rows
bit-equal inside a Ulysses group (B2), padding text content without effect (B3).

Processes: the ranks come from the fork server (the pytest process, which has the GPU open, starts no program itself); at most 8 ranks
+ this process on the card; all geometries of one world size run in one launch (six launches in all); init_process_group and every
gloo collective time out after a minute, the parent joins with a deadline and ends stragglers; a rank records a failed check and
still takes part in every remaining collective.

Largest replay error / fp64 bound per path (test_zz_ratio_report requires 0.05 < ratio <= 1 on each), measured on an MI355X:
    attn_fwd 0.542, attn_fwd long 0.178, ring 0.569, ring long 0.169
    (attn_fwd long carries the +90 of the static row bound in its gap, as the long cases of test_gpu_attention_edges.py do; ring long's
    gap is the largest over four half-chunk passes)
Largest error / tolerance of a sharded block against the oracle stage (rtol 2^-6, atol 6e-2), measured on an MI355X:
    double_block.0 img 0.198 / txt 0.199, single_block.0 img 0.159 / txt 0.103, single_block.1 img 0.103 / txt 0.102,
    final layer + output gather 0.164"""
import os

import pytest

pytestmark = pytest.mark.gpu

from tests import sp_wiring as S  # noqa: E402
from tests.sp_gpu_helpers import run_ranks  # noqa: E402

PATHS = ("attn_fwd", "attn_fwd long", "ring", "ring long")
RATIOS = {}


def _run(tmp_path, world, part, base):
    port = 29700 + base + world + (os.getpid() % 40)
    run_ranks(S.rank_main, world, (port, str(tmp_path), "cuda", part, None), start_method="forkserver", deadline=300.0)
    failures, ratios = S.read_results(str(tmp_path), world)
    for k, v in ratios.items():
        RATIOS[k] = max(RATIOS.get(k, 0.0), v)
    return failures, ratios


@pytest.mark.parametrize("world", S.WORLDS)
def test_attention_object_equals_single_rank_replay(world, tmp_path):
    failures, ratios = _run(tmp_path, world, "attention", 0)
    print(f"[sp wiring] world {world}: replay error / fp64 bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("world", S.MODEL_WORLDS)
def test_sharded_model_stage_by_stage(world, tmp_path):
    failures, ratios = _run(tmp_path, world, "model", 50)
    print(f"[sp wiring] world {world}: error / tolerance per stage: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert not failures, "\n".join(failures)


def test_zz_ratio_report(capsys):
    with capsys.disabled():
        print("\nsequence parallel: largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(RATIOS.items())))
    for p in PATHS:
        assert p in RATIOS, f"path {p} was never measured (run the whole file)"
        assert 0.05 < RATIOS[p] <= 1.0, f"{p}: ratio {RATIOS[p]:.3g} (a bound looser than 0.05 catches nothing)"
    stages = {k: v for k, v in RATIOS.items() if k.startswith("B1 ")}
    assert stages and all(v <= 1.0 for v in stages.values()), stages
