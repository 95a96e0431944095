"""CPU only: known answers of the numpy restatement tests/motion_ref.py (the double the GPU tests hold csrc/hv_motion.hip to), the host
rules of metrics.motion_from_host / motion_compare_fields / motion_summary on hand-made fields, the bucket labels, and the drivers'
flags."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _lib, metrics
from tests import content_ref, motion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script(rel):
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3] + "_motion_cpu", os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clip_of_bytes(q):
    """bytes [T, H, W] -> float32 [3, T, H, W] in [-1, 1] whose gray frames are q"""
    x = ((np.asarray(q, dtype=np.float64) + 0.5) / 255.0 * 2.0 - 1.0).astype(np.float16).astype(np.float32)
    return np.broadcast_to(x[None], (3, *x.shape)).copy()


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(3, -5), (-8, 8)], ids=str)
def test_a_shifted_texture_is_found_exactly(shift):
    H, W, B, R = 37, 50, 16, 8
    sy, sx = shift
    P = np.random.default_rng(5).integers(0, 256, size=(H, W))
    mv, sad, sad0 = ref.block_motion_of_gray(np.stack([P, ref.shifted(P, sy, sx)]), B, R)
    assert mv.shape == (1, 3, 4, 2) and mv.dtype == np.int16 and sad.dtype == sad0.dtype == np.uint32
    assert not sad.any() and sad0.all()
    for by in range(3):
        for bx in range(4):
            rows, cols = range(by * B, min(by * B + B, H)), range(bx * B, min(bx * B + B, W))
            inside = all(0 <= y + sy < H for y in rows) and all(0 <= x + sx < W for x in cols)
            if inside:
                assert tuple(mv[0, by, bx]) == (sy, sx), (by, bx)
    if shift == (-8, 8):
        # the 2-column block at the clamped side: its matched columns are all the frame's last one, every dx >= 1 gives SAD 0 and the tie
        # goes to the shorter vector
        assert mv[0, 0, 3, 1] == 1 and mv[0, 1, 3, 1] == 1


def test_constant_and_striped_frames_stay_put():
    for B in (8, 16):
        mv, sad, sad0 = ref.block_motion_of_gray(np.full((3, 20, 33), 91), B, 6)
        assert not mv.any() and not sad.any() and not sad0.any() and mv.shape == (2, -(-20 // B), -(-33 // B), 2)
        g = np.broadcast_to((np.arange(33) % 4) * 60, (2, 20, 33))
        mv, sad, sad0 = ref.block_motion_of_gray(g, B, 6, lam=0)        # dx = +-4 match as well: the norm breaks the tie
        assert not mv.any() and not sad.any() and not sad0.any()


def test_a_large_lam_pulls_vectors_to_zero():
    P = np.random.default_rng(6).integers(100, 104, size=(32, 32))      # a faint texture: moving gains at most 3 codes a pixel
    g = np.stack([P, ref.shifted(P, 1, 2)])
    free = ref.block_motion_of_gray(g, 16, 4, lam=0)
    held = ref.block_motion_of_gray(g, 16, 4, lam=255)
    assert tuple(free[0][0, 0, 0]) == (1, 2) and free[1][0, 0, 0] == 0
    assert not held[0].any() and (held[1] == held[2]).all() and (free[2] == held[2]).all()


def test_saturated_frames_do_not_wrap():
    g = np.stack([np.zeros((16, 24)), np.full((16, 24), 255)])
    mv, sad, sad0 = ref.block_motion_of_gray(g, 16, 3)
    assert not mv.any() and sad.tolist() == [[[16 * 16 * 255, 16 * 8 * 255]]] and (sad == sad0).all()


def test_a_single_frame_has_no_rows_and_the_float_path_quantises_as_the_content_reference():
    mv, sad, sad0 = ref.block_motion_of_gray(np.zeros((1, 9, 9)), 8, 2)
    assert mv.shape == (0, 2, 2, 2) and sad.shape == sad0.shape == (0, 2, 2)
    q = np.random.default_rng(7).integers(0, 256, size=(2, 9, 12))
    x = _clip_of_bytes(q)
    assert (content_ref.gray_frames(x).reshape(2, 9, 12) == q).all()
    for a, b in zip(ref.block_motion(x, 8, 3), ref.block_motion_of_gray(q, 8, 3)):
        assert (a == b).all()
    assert ref.default_lam(16) == 16 and ref.default_lam(8) == 4 and metrics.motion_default_lam(16) == 16 and metrics.motion_default_lam(8) == 4


# ---- the host rules ------------------------------------------------------------------------------------------------------------------------
def _field(mv, sad, sad0, radius=4, block=16, lam=16):
    return {"mv": np.asarray(mv, dtype=np.int16), "sad": np.asarray(sad, dtype=np.int32), "sad0": np.asarray(sad0, dtype=np.int32),
            "block": block, "radius": radius, "lam": lam}


def test_motion_from_host_on_a_hand_made_field():
    mv = np.zeros((2, 2, 2, 2), dtype=np.int16)
    mv[0, 0, 0] = (3, 4)
    mv[0, 1, 1] = (0, -4)
    mv[1, 0, 1] = (-1, 0)
    sad = np.array([[[1, 2], [3, 4]], [[0, 0], [0, 10]]])
    sad0 = 4 * sad + 5
    d = metrics.motion_from_host(mv, sad, sad0, 4, 16, 16)
    assert d["motion_pairs"] == [(5.0 + 4.0) / 4, 0.25] and d["motion_mean"] == ((5.0 + 4.0) / 4 + 0.25) / 2
    assert d["motion_max"] == 5.0 and d["static_share"] == 5 / 8 and d["border_share"] == 2 / 8
    assert d["mc_gain"] == 1.0 - 20 / 120 and d["frames"] == 3 and (d["block"], d["radius"], d["lam"]) == (16, 4, 16)
    assert d["definition"] == metrics.MOTION_DEFINITION == ref.DEFINITION
    assert "not FVMD" in d["definition"] and "this project's own" in d["definition"]
    json.dumps(d)
    flat = metrics.motion_from_host(np.zeros((1, 1, 1, 2)), [[[0]]], [[[0]]], 8)
    assert flat["mc_gain"] == 0.0 and flat["motion_mean"] == 0.0 and flat["static_share"] == 1.0 and flat["border_share"] == 0.0
    none = metrics.motion_from_host(np.zeros((0, 2, 2, 2)), np.zeros((0, 2, 2)), np.zeros((0, 2, 2)), 8, 16, 16)
    assert none["frames"] == 1 and none["motion_pairs"] == [] and none["definition"] == metrics.MOTION_DEFINITION
    assert all(none[k] is None for k in ("motion_mean", "motion_max", "static_share", "border_share", "mc_gain"))


def test_compare_and_summary_on_hand_made_fields():
    a = np.zeros((3, 1, 2, 2), dtype=np.int16)
    a[:, 0, 0] = (3, 4)
    b = np.zeros((2, 1, 2, 2), dtype=np.int16)
    b[:, 0, 0] = (0, 4)
    ones = lambda n: np.ones((n, 1, 2))      # noqa: E731
    fa, fb = _field(a, ones(3), 2 * ones(3)), _field(b, ones(2), 2 * ones(2))
    c = metrics.motion_compare_fields(fa, fb)
    assert c["ref"]["frames"] == c["rec"]["frames"] == 3              # the pairs both have
    assert c["motion_epe"] == 1.5 and c["ref"]["motion_mean"] == 2.5 and c["rec"]["motion_mean"] == 2.0 and c["motion_mean_change"] == -0.5
    assert metrics.motion_epe(a, a) == 0.0 and metrics.motion_epe(a[:0], a[:0]) is None
    with pytest.raises(ValueError):
        metrics.motion_epe(a, b)
    with pytest.raises(ValueError, match="geometry"):
        metrics.motion_compare_fields(fa, _field(b, ones(2), ones(2), radius=8))
    single = metrics.motion_compare_fields(_field(a[:0], ones(0), ones(0)), fb)
    assert single["motion_epe"] is None and single["motion_mean_change"] is None
    s = metrics.motion_summary([metrics.motion_field_stats(fa), metrics.motion_field_stats(_field(a[:0], ones(0), ones(0)))], [c, single])
    assert s["clips"] == 2 and s["input"]["motion_mean"] == 2.5 and s["reconstruction"]["motion_mean"] == 2.0 and s["motion_epe"] == 1.5
    assert s["motion_mean_change"] == -0.5 and (s["block"], s["radius"], s["lam"]) == (16, 4, 16) and s["definition"] == metrics.MOTION_DEFINITION
    json.dumps(s)
    empty = metrics.motion_summary([], [])
    assert empty["clips"] == 0 and empty["motion_epe"] is None


def test_the_accumulator_gains_motion_lines_only_when_asked(tmp_path):
    acc = metrics.MetricsAccumulator()
    acc.add([30.0], [0.9])
    assert set(acc.result()) == {"PSNR", "SSIM"}
    a = np.zeros((1, 1, 1, 2), dtype=np.int16)
    b = a.copy()
    b[0, 0, 0] = (0, 2)
    acc.add_motion(metrics.motion_compare_fields(_field(a, [[[1]]], [[[1]]]), _field(b, [[[1]]], [[[3]]])))
    res = acc.result()
    assert res["MotionEPE"] == 2.0 and res["MotionMean"] == 2.0 and list(res) == ["PSNR", "SSIM", "MotionEPE", "MotionMean"]
    text = open(acc.save(str(tmp_path), "r1", "r2")).read()
    assert "\nMotionEPE: 2.0 (" in text and "\nMotionMean: 2.0 (" in text and "not FVMD" in text
    assert metrics.METRICS_CSV_HEADER == ["video_path", "ssim", "psnr", "lpips", "fvd", "fvdm"]


def test_parameters_and_cpu_tensors_are_refused():
    x = torch.zeros(3, 2, 4, 4)
    for fn in (metrics.block_motion, metrics.motion_stats):
        with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
            fn(x)
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.motion_compare(x, x)
    for kw in (dict(block=12), dict(radius=0), dict(radius=33), dict(lam=-1), dict(lam=256)):
        args = dict(block=16, radius=16, lam=None)
        args.update(kw)
        with pytest.raises(ValueError):
            metrics._motion_params(**args)
    assert metrics._motion_params(8, 32, None) == (8, 32, 4) and metrics._motion_params(16, 1, 255) == (16, 1, 255)
    assert metrics.motion_stats_many([]) == []


# ---- buckets and drivers -------------------------------------------------------------------------------------------------------------------
def test_bucket_labels():
    assert metrics.content_bucket_labels((1, 4, 8), "motion") == ["Very_Low_Motion_lt1", "Low_Motion_1-4", "Medium_Motion_4-8", "High_Motion_gt8"]
    assert metrics.content_bucket_labels((0.5,), "motion") == ["B0_Motion_lt0.5", "B1_Motion_gt0.5"]
    assert metrics.content_bucket(4.0, (1, 4, 8), "motion") == "Medium_Motion_4-8" and metrics.content_bucket(None, (1,), "motion") is None
    # the existing calls give the strings they gave
    assert metrics.content_bucket_labels() == ["Very_Low_InterEntropy_lt2", "Low_InterEntropy_2-4", "Medium_InterEntropy_4-6", "High_InterEntropy_gt6"]
    assert metrics.content_bucket(7.5, metric="intra") == "High_IntraEntropy_gt6"
    with pytest.raises(ValueError, match="'inter', 'intra' or 'motion'"):
        metrics.content_bucket_labels((1,), "bitrate")


def _motion_double(dataset, n, params):
    """the numpy stand-in for tools/bucket_clips.motion_on_gpu"""
    out = []
    for i in range(n):
        f = ref.block_motion(np.asarray(dataset[i][0], dtype=np.float32), params["block"], params["radius"], params["lam"])
        out.append(metrics.motion_from_host(*f, params["radius"], params["block"], params["lam"]))
    return out


def test_bucket_clips_by_motion(tmp_path, capsys):
    tool = _load_script("tools/bucket_clips.py")
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    P = np.random.default_rng(9).integers(0, 256, size=(24, 24))
    q = {"a_still": np.stack([P, P, P]), "b_pan": np.stack([P, ref.shifted(P, 0, 3), ref.shifted(ref.shifted(P, 0, 3), 0, 3)]), "c_single": P[None]}
    for name, v in q.items():
        torch.save(torch.from_numpy(_clip_of_bytes(v)), str(src / (name + ".pt")))
    argv = ["--tensor-dir", str(src), "--output-dir", str(out), "--metric", "motion", "--edges", "1", "--motion-block", "8", "--motion-radius", "4"]
    recs = tool.main(argv, measure_motion=_motion_double)
    printed = capsys.readouterr().out
    assert [json.loads(ln) for ln in open(out / "motion.jsonl")] == recs and not os.path.exists(out / "content.jsonl")
    by = {r["name"]: r for r in recs}
    assert by["a_still"]["bucket"] == "B0_Motion_lt1" and by["a_still"]["value"] == 0.0
    assert by["b_pan"]["bucket"] == "B1_Motion_gt1" and by["b_pan"]["value"] == by["b_pan"]["motion_mean"] > 2.0
    assert by["c_single"]["bucket"] is None and by["c_single"]["motion_mean"] is None
    assert all(r["metric"] == "motion" and r["definition"] == metrics.MOTION_DEFINITION and (r["block"], r["radius"], r["lam"]) == (8, 4, 4) for r in recs)
    assert sorted(f for f in os.listdir(out) if f.endswith(".txt")) == ["B0_Motion_lt1.txt", "B1_Motion_gt1.txt"]
    assert "px/frame" in printed and "not FVMD" in printed and "c_single" in printed


@pytest.mark.parametrize("argv,msg", [
    (["--metric", "motion"], "needs --edges"), (["--motion-radius", "8"], "only valid with --metric motion"),
    (["--metric", "motion", "--edges", "1", "--motion-radius", "33"], "radius is in [1, 32]"),
    (["--metric", "motion", "--edges", "1", "--motion-block", "12"], "invalid choice"),
    (["--metric", "motion", "--edges", "1", "--motion-lam", "256"], "lam is in [0, 255]"),
    (["--metric", "motion", "--edges", "3", "2"], "ascending"), (["--metric", "motion", "--edges", "30"], "px/frame"),
], ids=lambda v: "-".join(v) if isinstance(v, list) else None)
def test_bucket_clips_motion_argument_errors(tmp_path, capsys, argv, msg):
    tool = _load_script("tools/bucket_clips.py")
    (tmp_path / "in").mkdir()
    with pytest.raises(SystemExit):
        tool.main(["--tensor-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out")] + argv, measure_motion=_motion_double)
    assert msg in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")


def test_driver_flags(tmp_path, capsys):
    t_ops = os.path.join(ROOT, "tests", "golden", "t_ops_config.json")
    base = ["--tensor-dir", str(tmp_path), "--output-dir", str(tmp_path / "o")]
    infer = _load_script("infer.py")
    study = _load_script("tools/run_vae_study.py")
    cm = _load_script("evaluation/compute_metrics.py")
    cm_base = ["--root1", str(tmp_path), "--root2", str(tmp_path), "--results-dir", str(tmp_path / "r")]
    # without the flags nothing changes
    assert infer.parse_args(base + ["--score"]).motion_params is None and study.parse_args(base + ["--base-config", t_ops]).motion_params is None
    assert cm.parse_args(cm_base).motion_params is None
    # the defaults and explicit values
    assert infer.parse_args(base + ["--score", "--motion"]).motion_params == {"block": 16, "radius": 16, "lam": 16}
    got = study.parse_args(base + ["--base-config", t_ops, "--motion", "--motion-block", "8", "--motion-radius", "32"]).motion_params
    assert got == {"block": 8, "radius": 32, "lam": 4}
    assert cm.parse_args(cm_base + ["--motion", "--motion-lam", "0"]).motion_params == {"block": 16, "radius": 16, "lam": 0}
    cases = [(infer.parse_args, base + ["--motion"], "--motion is only valid with --score"),
             (infer.parse_args, base + ["--score", "--motion-block", "8"], "--motion-block only valid with --motion"),
             (infer.parse_args, base + ["--score", "--motion", "--motion-radius", "0"], "radius is in [1, 32]"),
             (study.parse_args, base + ["--base-config", t_ops, "--motion-radius", "8", "--motion-lam", "1"],
              "--motion-radius, --motion-lam only valid with --motion"),
             (study.parse_args, base + ["--base-config", t_ops, "--motion", "--motion-lam", "300"], "lam is in [0, 255]"),
             (cm.parse_args, cm_base + ["--motion-lam", "3"], "--motion-lam only valid with --motion"),
             (cm.parse_args, cm_base + ["--motion", "--motion-block", "32"], "invalid choice")]
    for parse, argv, msg in cases:
        with pytest.raises(SystemExit):
            parse(argv)
        assert msg in capsys.readouterr().err, (argv, msg)
