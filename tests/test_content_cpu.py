"""Content statistics and buckets without a GPU: known answers of the numpy reference (tests/content_ref.py), the host rules of
metrics.content_from_host / content_bucket against it, and the drivers (tools/bucket_clips.py, tools/run_vae_study.py --bucket-dir) on
the numpy double in place of the device."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _lib, metrics
from tests import content_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hv_content_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _clip_of_bytes(q):
    """bytes [T, H, W] -> float32 [3, T, H, W] in [-1, 1] that quantises back to q in every channel (gray = q: the luma weights sum to
    2^15)"""
    x = (np.asarray(q, dtype=np.float64) + 0.5) / 255.0 * 2.0 - 1.0
    x = np.broadcast_to(x.astype(np.float32)[None], (3,) + np.asarray(q).shape).copy()
    assert (ref.gray_frames(x) == np.asarray(q).reshape(q.shape[0], -1)).all()
    return x


def _checkerboard(T, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    board = ((yy + xx) & 1) * 255
    return np.stack([board if t % 2 == 0 else 255 - board for t in range(T)])


# ---- known answers of the reference ---------------------------------------------------------------------------------------------------
def test_constant_clip_has_no_entropy():
    d = ref.content_entropy(_clip_of_bytes(np.full((4, 5, 7), 93)))
    assert d["intra_entropy"] == 0.0 and d["inter_entropy"] == 0.0 and d["mean_abs_diff"] == 0.0 and d["ti"] == 0.0 and d["frames"] == 4
    intra, inter = ref.histograms(_clip_of_bytes(np.full((4, 5, 7), 93)))
    assert (intra[:, 93] == 35).all() and intra.sum() == 4 * 35 and (inter[:, 255] == 35).all() and inter.sum() == 3 * 35


@pytest.mark.parametrize("hw", [(4, 6), (3, 5)], ids=["even", "odd"])
def test_inverting_checkerboard_is_one_bit_between_frames(hw):
    H, W = hw
    q = _checkerboard(3, H, W)
    d = ref.content_entropy(_clip_of_bytes(q))
    intra, inter = ref.histograms(_clip_of_bytes(q))
    assert (inter[:, 0] + inter[:, 510] == H * W).all() and inter.sum() == 2 * H * W
    if (H * W) % 2 == 0:
        assert d["inter_entropy"] == 1.0 and d["intra_entropy"] == 1.0
        assert d["inter_entropy_pairs"] == [1.0, 1.0] and d["mean_abs_diff"] == 255.0 and d["ti"] == 255.0
    else:                                                   # 8 cells of one colour, 7 of the other: just below one bit
        p = np.array([8, 7]) / 15.0
        assert abs(d["inter_entropy"] - float(-(p * np.log2(p)).sum())) < 1e-12 and d["inter_entropy"] < 1.0


def test_uniform_ramp_is_eight_bits_within_a_frame():
    q = np.arange(256).reshape(1, 16, 16).repeat(2, axis=0)
    d = ref.content_entropy(_clip_of_bytes(q))
    assert d["intra_entropy"] == 8.0 and d["inter_entropy"] == 0.0


def test_black_and_white_frames_in_alternation():
    q = np.stack([np.full((3, 4), 255 * (t % 2)) for t in range(4)])
    intra, inter = ref.histograms(_clip_of_bytes(q))
    d = ref.content_entropy(_clip_of_bytes(q))
    assert d["inter_entropy"] == 0.0 and d["intra_entropy"] == 0.0
    assert inter[0, 510] == 12 and inter[1, 0] == 12 and inter[2, 510] == 12 and inter.sum() == 36
    assert d["mean_abs_diff"] == 255.0 and d["ti"] == 0.0  # every pixel moves by the same amount: no spatial spread


def test_a_single_frame_has_no_inter_entropy():
    d = ref.content_entropy(_clip_of_bytes(np.arange(12).reshape(1, 3, 4)))
    assert d["inter_entropy"] is None and d["mean_abs_diff"] is None and d["ti"] is None and d["inter_entropy_pairs"] == []
    assert abs(d["intra_entropy"] - np.log2(12)) < 1e-12


def test_special_values_follow_the_quantiser():
    v = np.array([np.nan, np.inf, -np.inf, -3.0, 3.0, -1.0, 1.0, 0.0], dtype=np.float32)
    assert ref.quantised_gray(v, True).tolist() == [0, 255, 0, 0, 255, 0, 255, 127]
    assert ref.quantised_gray(v, False).tolist() == [0, 255, 0, 0, 255, 0, 255, 0]
    x = np.broadcast_to(v.reshape(1, 2, 1, 4), (3, 2, 1, 4)).copy()
    intra, inter = ref.histograms(x)
    assert intra[0, 0] == 3 and intra[0, 255] == 1 and intra[1].tolist().count(0) == 253
    # frame 1 - frame 0: 255 - 0, 0 - 255, 255 - 0, 127 - 0
    assert inter[0, 510] == 2 and inter[0, 0] == 1 and inter[0, 255 + 127] == 1


def test_row_stats_on_hand_made_rows():
    rows = np.zeros((4, 511), dtype=np.int64)
    rows[1, 17] = 1000                                      # a single bin
    rows[2, :] = 3                                          # all 511 bins equal
    rows[3, 0], rows[3, 510] = 5, 5
    s = ref.row_stats(rows, 255)
    assert s[0].tolist() == [0.0, 0.0, 0.0]
    assert s[1].tolist() == [0.0, 1000.0 * (17 - 255), 1000.0 * (17 - 255) ** 2]
    assert abs(s[2, 0] - np.log2(511)) < 1e-12 and s[2, 1] == 0.0 and s[2, 2] == 3.0 * 2 * sum(k * k for k in range(1, 256))
    assert s[3].tolist() == [1.0, 0.0, 10.0 * 255 ** 2]


# ---- the host rules of the package against the reference -------------------------------------------------------------------------------
def test_content_from_host_equals_the_reference_field_by_field():
    rng = np.random.default_rng(5)
    for T in (1, 2, 5):
        g = rng.integers(0, 256, size=(T, 77))
        if T == 5:
            g[3] = g[2]                                     # a repeated frame: a pair without entropy
        intra, inter = ref.histograms_of_gray(g)
        got = metrics.content_from_host(ref.row_stats(intra, 0), ref.row_stats(inter, 255), inter, T, 77)
        want = ref.content_of_gray(g)
        assert set(got) == set(want)
        for k, v in want.items():
            if isinstance(v, float):
                assert abs(got[k] - v) <= ref.ENTROPY_TOL, (T, k, got[k], v)
            elif isinstance(v, list):
                assert np.allclose(got[k], v, rtol=0, atol=ref.ENTROPY_TOL) and len(got[k]) == len(v), (T, k)
            else:
                assert got[k] == v, (T, k)
    assert metrics.CONTENT_DEFINITION == ref.DEFINITION and "this project's definition" in ref.DEFINITION
    assert metrics.CONTENT_INTER_BINS == ref.INTER_BINS


def test_content_summary_averages_over_clips_and_skips_single_frames():
    a = ref.content_of_gray(np.array([[0, 1, 2, 3], [3, 2, 1, 0]]))
    b = ref.content_of_gray(np.array([[5, 5, 5, 5]]))        # one frame: no inter-frame entropy
    s = metrics.content_summary([a, b], [b, b])
    assert s["input"]["inter_entropy"] == a["inter_entropy"] == 2.0 and s["reconstruction"]["inter_entropy"] is None
    assert s["inter_entropy_drop"] is None and s["clips"] == 2 and s["definition"] == ref.DEFINITION
    assert s["input"]["intra_entropy"] == (a["intra_entropy"] + b["intra_entropy"]) / 2
    assert metrics.content_summary([a], [ref.content_of_gray(np.array([[0, 1, 2, 3], [0, 1, 2, 3]]))])["inter_entropy_drop"] == 2.0


# ---- the bucket rule ----------------------------------------------------------------------------------------------------------------------
def test_bucket_edges_are_half_open_and_the_names_are_the_forks():
    assert [b[0] for b in metrics.CONTENT_BUCKETS] == list(ref.LABELS)
    assert [b[0] for b in metrics.CONTENT_BUCKETS[:3]] == ["Very_Low_InterEntropy_lt2", "Low_InterEntropy_2-4", "Medium_InterEntropy_4-6"]
    assert [(lo, hi) for _, lo, hi in metrics.CONTENT_BUCKETS] == [(None, 2.0), (2.0, 4.0), (4.0, 6.0), (6.0, None)]
    assert metrics.content_bucket(2.0) == "Low_InterEntropy_2-4" and metrics.content_bucket(4.0) == "Medium_InterEntropy_4-6"
    assert metrics.content_bucket(6.0) == "High_InterEntropy_gt6" and metrics.content_bucket(np.nextafter(2.0, 0.0)) == "Very_Low_InterEntropy_lt2"
    assert metrics.content_bucket(0.0) == "Very_Low_InterEntropy_lt2" and metrics.content_bucket(8.9) == "High_InterEntropy_gt6"
    assert metrics.content_bucket(None) is None and ref.bucket(None) is None
    for v in (0.0, 1.999, 2.0, 3.0, 4.0, 5.5, 6.0, 7.0):
        assert metrics.content_bucket(v) == ref.bucket(v), v
    assert metrics.content_bucket(1.0, edges=(1, 3.5)) == "B1_InterEntropy_1-3.5" and metrics.content_bucket(0.5, edges=(1, 3.5)) == "B0_InterEntropy_lt1"
    assert metrics.content_bucket(3.5, edges=(1, 3.5)) == "B2_InterEntropy_gt3.5"
    assert metrics.content_bucket(7.5, metric="intra") == "High_IntraEntropy_gt6"
    with pytest.raises(ValueError):
        metrics.content_bucket(1.0, edges=(4, 2))
    with pytest.raises(ValueError):
        metrics.content_bucket(1.0, edges=())


def test_cpu_tensors_are_refused():
    x = torch.zeros(3, 2, 4, 4)
    for fn in (metrics.content_histograms, metrics.content_entropy):
        with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
            fn(x)
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.histogram_entropy(torch.zeros(2, 256, dtype=torch.int32))


# ---- the drivers on the numpy double ------------------------------------------------------------------------------------------------------
def _clips(folder):
    """four clips: static (0 bits), a two-level flicker (1 bit), noise on 32 levels (about 5.5 bits), full-range noise (above 6)"""
    rng = np.random.default_rng(11)
    q = {"a_static": np.full((3, 8, 8), 40), "b_flicker": _checkerboard(3, 8, 8),
         "c_mid": rng.integers(100, 132, size=(3, 32, 32)), "d_noise": rng.integers(0, 256, size=(3, 32, 32)), "e_single": np.full((1, 8, 8), 7)}
    os.makedirs(folder, exist_ok=True)
    for name, v in q.items():
        torch.save(torch.from_numpy(_clip_of_bytes(v)), os.path.join(folder, name + ".pt"))
    return q


def test_bucket_clips_writes_records_lists_and_summaries(tmp_path, capsys):
    tool = _load_script("tools/bucket_clips.py")
    src, out = str(tmp_path / "in"), str(tmp_path / "out")
    q = _clips(src)
    recs = tool.main(["--tensor-dir", src, "--output-dir", out], measure=ref.measure)
    printed = capsys.readouterr().out
    assert [json.loads(ln) for ln in open(os.path.join(out, "content.jsonl"))] == recs and len(recs) == 5
    by = {r["name"]: r for r in recs}
    assert by["a_static"]["bucket"] == by["b_flicker"]["bucket"] == "Very_Low_InterEntropy_lt2"
    assert by["b_flicker"]["inter_entropy"] == 1.0 and by["a_static"]["inter_entropy"] == 0.0
    assert by["c_mid"]["bucket"] == "Medium_InterEntropy_4-6" and by["d_noise"]["bucket"] == "High_InterEntropy_gt6"
    assert by["e_single"]["bucket"] is None and by["e_single"]["inter_entropy"] is None
    for r in recs:
        want = ref.content_of_gray(q[r["name"]].reshape(q[r["name"]].shape[0], -1))
        assert all(r[k] == want[k] for k in want) and r["definition"] == ref.DEFINITION and r["metric"] == "inter"
        assert r["file"] == os.path.join(src, r["name"] + ".pt") and r["value"] == r["inter_entropy"]
    lists = sorted(f for f in os.listdir(out) if f.endswith(".txt"))
    assert lists == ["High_InterEntropy_gt6.txt", "Medium_InterEntropy_4-6.txt", "Very_Low_InterEntropy_lt2.txt"]      # Low is empty: no file
    assert open(os.path.join(out, "Very_Low_InterEntropy_lt2.txt")).read() == "".join(os.path.join(src, n) + "\n" for n in ("a_static.pt", "b_flicker.pt"))
    assert "Very_Low_InterEntropy_lt2: 2 clips" in printed and "High_InterEntropy_gt6: 1 clips" in printed and "e_single" in printed
    assert "Low_InterEntropy_2-4" not in printed
    # custom edges, the intra metric and --max-files
    recs = tool.main(["--tensor-dir", src, "--output-dir", str(tmp_path / "o2"), "--metric", "intra", "--edges", "0.5", "--max-files", "3"],
                     measure=ref.measure)
    assert [r["bucket"] for r in recs] == ["B0_IntraEntropy_lt0.5", "B1_IntraEntropy_gt0.5", "B1_IntraEntropy_gt0.5"]
    assert sorted(f for f in os.listdir(tmp_path / "o2") if f.endswith(".txt")) == ["B0_IntraEntropy_lt0.5.txt", "B1_IntraEntropy_gt0.5.txt"]


@pytest.mark.parametrize("argv,msg", [
    (["--edges", "4", "2"], "ascending"), (["--edges", "2", "2"], "ascending"), (["--edges", "0"], "between 0 and 16"),
    (["--metric", "bitrate"], "invalid choice"), (["--max-files", "0"], "positive"), (["--target-height", "240"], "yuv"),
], ids=lambda v: "-".join(v) if isinstance(v, list) else None)
def test_bucket_clips_argument_errors(tmp_path, capsys, argv, msg):
    tool = _load_script("tools/bucket_clips.py")
    (tmp_path / "in").mkdir()
    with pytest.raises(SystemExit):
        tool.main(["--tensor-dir", str(tmp_path / "in"), "--output-dir", str(tmp_path / "out")] + argv, measure=ref.measure)
    assert msg in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "out")


def test_bucket_clips_refuses_a_missing_or_empty_folder(tmp_path, capsys):
    tool = _load_script("tools/bucket_clips.py")
    with pytest.raises(SystemExit):
        tool.main(["--tensor-dir", str(tmp_path / "nowhere"), "--output-dir", str(tmp_path / "out")], measure=ref.measure)
    assert "is not a folder" in capsys.readouterr().err
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit, match="no clips"):
        tool.main(["--tensor-dir", str(tmp_path / "empty"), "--output-dir", str(tmp_path / "out")], measure=ref.measure)


def test_bucket_lists_match_by_stem_and_a_missing_clip_is_an_error(tmp_path):
    study = _load_script("tools/run_vae_study.py")
    files = ["a.pt", "b.pt", "c_30fps_64x64.yuv"]
    bd = tmp_path / "buckets"
    bd.mkdir()
    (bd / "Very_Low_InterEntropy_lt2.txt").write_text("/videos/elsewhere/b.mp4\n\na.pt\n")       # the fork's lists name .mp4 files
    (bd / "Low_InterEntropy_2-4.txt").write_text("some/dir/c_30fps_64x64.yuv\nb\nb.pt\n")
    (bd / "notes.md").write_text("not a list")
    got = study.read_bucket_lists(str(bd), files)
    assert got == [("Low_InterEntropy_2-4", [2, 1]), ("Very_Low_InterEntropy_lt2", [1, 0])]          # sorted by list name, clips in list order
    (bd / "Medium_InterEntropy_4-6.txt").write_text("a.pt\nzz.mp4\n")
    with pytest.raises(ValueError, match="zz"):
        study.read_bucket_lists(str(bd), files)
    (bd / "Medium_InterEntropy_4-6.txt").write_text("\n")
    with pytest.raises(ValueError, match="empty"):
        study.read_bucket_lists(str(bd), files)
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(ValueError, match="no <bucket>.txt"):
        study.read_bucket_lists(str(empty), files)


def test_clip_subset_keeps_the_dataset_surface():
    study = _load_script("tools/run_vae_study.py")

    class DS:
        tensor_files = ["a.pt", "b.pt", "c.pt"]
        fps = {"b.pt": 30}

        def __getitem__(self, i):
            return i * 10, self.tensor_files[i]

        def __len__(self):
            return 3
    sub = study.ClipSubset(DS(), [2, 0])
    assert len(sub) == 2 and sub[0] == (20, "c.pt") and sub[1] == (0, "a.pt") and sub.tensor_files == ["c.pt", "a.pt"] and sub.fps == {"b.pt": 30}


def test_study_argument_errors_for_the_new_flags(tmp_path, capsys):
    study = _load_script("tools/run_vae_study.py")
    t_ops = os.path.join(ROOT, "tests", "golden", "t_ops_config.json")
    with pytest.raises(SystemExit):
        study.parse_args(["--tensor-dir", str(tmp_path), "--output-dir", str(tmp_path / "o"), "--base-config", t_ops, "--bucket-dir",
                          str(tmp_path / "nowhere")])
    assert "--bucket-dir" in capsys.readouterr().err
    a = study.parse_args(["--tensor-dir", str(tmp_path), "--output-dir", str(tmp_path / "o"), "--base-config", t_ops])
    assert a.bucket_dir is None and a.content is False
    infer = _load_script("infer.py")
    with pytest.raises(SystemExit):
        infer.parse_args(["--tensor-dir", str(tmp_path), "--output-dir", str(tmp_path / "o"), "--content"])
    assert "--content is only valid with --score" in capsys.readouterr().err
