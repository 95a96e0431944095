"""CPU, gloo: the checks of tests/sp_wiring.py on the REAL host code of the sequence-parallel path (long_ctx_attention.py, the segment
loops of modules/models.py, inference.parallelize_transformer_module) with the kernels replaced by the CPU doubles: (1) the faithful
code passes every check at every geometry (the two long ones need the HIP kernels' split rule and run on the GPU only); (2) every
mutant - a deliberately mis-wired exchange - is rejected, and the failure message names the check assigned to it.  No GPU."""
import os

import pytest

from tests import sp_wiring as S
from tests.sp_gpu_helpers import run_ranks


def _run(tmp_path, world, part, mutant=None, base=0):
    port = 29400 + base + world + (os.getpid() % 150)
    run_ranks(S.rank_main, world, (port, str(tmp_path), "cpu", part, mutant), start_method="spawn", deadline=300.0)
    return S.read_results(str(tmp_path), world)


@pytest.mark.parametrize("world", S.WORLDS)
def test_attention_object_equals_single_rank_replay(world, tmp_path):
    failures, ratios = _run(tmp_path, world, "attention")
    print(f"[sp wiring] world {world}: replay error / fp64 bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert not failures, "\n".join(failures)
    assert ratios and all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("world", S.MODEL_WORLDS)
def test_sharded_model_stage_by_stage(world, tmp_path):
    failures, ratios = _run(tmp_path, world, "model", base=200)
    print(f"[sp wiring] world {world}: error / tolerance per stage: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    assert not failures, "\n".join(failures)
    assert ratios and all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("name", list(S.MUTANTS))
def test_mutant_is_rejected(name, tmp_path):
    check, case = S.MUTANTS[name][0], S.MUTANTS[name][1]
    failures, _ = _run(tmp_path, case.world, "mutant", name, base=400 + 7 * list(S.MUTANTS).index(name))
    print(f"[sp wiring] mutant {name}: " + "\n".join(f[:300] for f in failures))
    assert failures, f"{name}: no check failed"
    assert any(f.startswith(check + ":") for f in failures), f"{name}: not rejected by {check}:\n" + "\n".join(failures)
    assert not any(f.startswith(("worker raised", "rank ", "faithful: ")) for f in failures), "\n".join(failures)
