"""bench.py's command line (CPU only): a plain run times its steps and prints the line; every leg that the headline figure does
not need runs only with --full, where each keeps its own opt-out."""
import bench


def _legs(argv, world=1):
    return bench.extra_legs(bench.build_parser().parse_args(argv), world)


def test_plain_run_adds_no_legs():
    for argv in ([], ["--gpus", "1", "--steps", "3", "--warmup", "1"], ["--workload", "544p65f"], ["--use-fp8", "--fp8-mfma"],
                 ["--dump-outputs", "out"]):
        assert not any(_legs(argv).values()), argv
    assert not any(_legs(["--gpus", "2"], world=2).values())


def test_full_run_adds_every_leg_of_the_default_workload():
    assert _legs(["--full"]) == {"secondary": True, "vae": True, "cpu_baseline": True}
    assert _legs(["--full", "--gpus", "1", "--steps", "20", "--warmup", "5"]) == {"secondary": True, "vae": True, "cpu_baseline": True}


def test_full_run_opt_outs_and_scope():
    assert _legs(["--full", "--no-secondary"]) == {"secondary": False, "vae": True, "cpu_baseline": True}
    assert _legs(["--full", "--no-vae"]) == {"secondary": True, "vae": False, "cpu_baseline": True}
    assert _legs(["--full", "--no-cpu-baseline"]) == {"secondary": True, "vae": True, "cpu_baseline": False}
    # the secondary workloads belong to the single-GPU bf16 720p129f line; the tiny model has no VAE leg; N > 1: VAE only
    assert _legs(["--full", "--workload", "544p65f"])["secondary"] is False
    assert _legs(["--full", "--use-fp8"])["secondary"] is False
    assert _legs(["--full", "--force-sp"])["secondary"] is False
    assert _legs(["--full", "--workload", "tiny"]) == {"secondary": False, "vae": False, "cpu_baseline": True}
    assert _legs(["--full", "--gpus", "2"], world=2) == {"secondary": False, "vae": True, "cpu_baseline": False}
