"""GPU: reconstruction scoring (csrc/hv_metrics.hip through metrics.video_metrics) against golden scores skimage produced
(tools/make_golden_metrics.py) and, where there is no golden vector, the float64 restatement tests/metrics_ref.py.

Bounds.  The quantised bytes, hence `sse`, `min`, `max`, are integers and must be EXACT.  PSNR is float64 host arithmetic on that
integer: 1e-9 dB.  SSIM: the box moments are exact integers, so the only error is the fp32 evaluation of the map value - about 16
roundings of 2^-24 each on a ratio whose numerator never exceeds its denominator in magnitude (vx + vy + C2 >= |2 vxy + C2|), i.e.
~1e-6 per window position and so for their mean; the sums are fp64.  1e-5 absolute is that bound with a decade of margin."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _lib, metrics  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import metrics_ref  # noqa: E402
from tests.test_metrics_cpu import GOLDEN, ROOT, T_OPS, golden_pairs  # noqa: E402

DEV = "cuda:0"
PSNR_TOL = 1e-9
SSIM_TOL = 1e-5


def _strided(x, kind):
    """the same values behind another memory layout: `t` - every other frame of a longer buffer; `h` - rows of a taller, wider
    buffer (row stride > W, an odd element offset: no 16-byte alignment)"""
    C, T, H, W = x.shape
    if kind == "contiguous":
        return x.contiguous()
    if kind == "t":
        buf = torch.full((C, 2 * T, H, W), 0.25, dtype=x.dtype, device=x.device)
        buf[:, ::2] = x
        return buf[:, ::2]
    buf = torch.full((C, T, 2 * H + 1, W + 5), -0.5, dtype=x.dtype, device=x.device)
    buf[:, :, 1:2 * H:2, 3:3 + W] = x
    return buf[:, :, 1:2 * H:2, 3:3 + W]


def _check_pair(name, x1, x2, b1, b2, psnr, ssim, dtype, layout):
    ref = _strided(torch.from_numpy(x1).to(DEV, dtype)[:, None], layout)
    rec = _strided(torch.from_numpy(x2).to(DEV, dtype)[:, None], layout)
    m = metrics.video_metrics(ref, rec)
    d = b1.astype(np.int64) - b2.astype(np.int64)
    tag = (name, dtype, layout)
    print(f"{name} {dtype} {layout}: sse {int(m['sse'][0])} psnr err {abs(m['psnr'][0] - psnr):.3e} ssim err {abs(m['ssim'][0] - ssim):.3e}")
    assert int(m["sse"][0]) == int((d * d).sum()), tag
    assert m["minmax"][0].tolist() == [int(b1.min()), int(b1.max()), int(b2.min()), int(b2.max())], tag
    assert abs(m["psnr"][0] - psnr) <= PSNR_TOL, tag
    assert abs(m["ssim"][0] - ssim) <= SSIM_TOL, tag


@pytest.mark.parametrize("layout", ["contiguous", "t", "h"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_every_golden_pair(dtype, layout):
    pairs = golden_pairs()
    assert len(pairs) >= 40
    for p in pairs:
        _check_pair(*p, dtype, layout)


def test_golden_pairs_stacked_as_frames_of_one_video():
    """the 15 pairs of one size as 15 frames: every frame gets its own data range, constants and the PSNR-100 rule"""
    pairs = [p for p in golden_pairs() if p[0].startswith("7x40x3_")]
    ref = torch.from_numpy(np.stack([p[1] for p in pairs], 1)).to(DEV)
    rec = torch.from_numpy(np.stack([p[2] for p in pairs], 1)).to(DEV)
    m = metrics.video_metrics(ref, rec)
    assert m["psnr"].shape == (len(pairs),) and m["psnr"].dtype == np.float64
    for t, p in enumerate(pairs):
        assert abs(m["psnr"][t] - p[5]) <= PSNR_TOL and abs(m["ssim"][t] - p[6]) <= SSIM_TOL, p[0]
    assert m["psnr_mean"] == pytest.approx(np.mean([p[5] for p in pairs]), abs=1e-9)


def _video(shape, key):
    x = syn.hashed_uniform(shape, key, 0)
    x = x / x.abs().max()
    return x.half()


def test_tile_edges_against_float64_restatement():
    """3 x 5 x 131 x 263: several tiles each way, the last ones ragged"""
    a = _video((3, 5, 131, 263), "metrics.edge.a")
    b = (a.float() + 0.08 * _video((3, 5, 131, 263), "metrics.edge.b").float()).half()
    b[:, 3] = a[:, 3]                                       # one identical frame
    ps, ss = metrics_ref.video_scores(a.float().numpy(), b.float().numpy())
    for dtype in (torch.float16, torch.float32):
        m = metrics.video_metrics(a.to(DEV, dtype), b.to(DEV, dtype))
        qa, qb = metrics_ref.quantise(a.float().numpy()).astype(np.int64), metrics_ref.quantise(b.float().numpy()).astype(np.int64)
        print(f"edges {dtype}: psnr err {np.abs(m['psnr'] - ps).max():.3e} ssim err {np.abs(m['ssim'] - ss).max():.3e}")
        assert m["sse"].tolist() == ((qa - qb) ** 2).sum(axis=(0, 2, 3)).tolist()
        assert m["minmax"][:, 0].tolist() == qa.min(axis=(0, 2, 3)).tolist() and m["minmax"][:, 3].tolist() == qb.max(axis=(0, 2, 3)).tolist()
        assert np.abs(m["psnr"] - ps).max() <= PSNR_TOL and m["psnr"][3] == 100.0
        assert np.abs(m["ssim"] - ss).max() <= SSIM_TOL


def test_rescale_off_reads_unit_range():
    a = _video((3, 2, 20, 33), "metrics.unit.a").float().abs()
    b = (a * 0.9).contiguous()
    ps, ss = metrics_ref.video_scores(a.numpy(), b.numpy(), rescale=False)
    m = metrics.video_metrics(a.to(DEV), b.to(DEV), rescale=False)
    assert np.abs(m["psnr"] - ps).max() <= PSNR_TOL and np.abs(m["ssim"] - ss).max() <= SSIM_TOL


def test_two_calls_give_identical_bits_and_batch_rows_equal_single_calls():
    a = torch.stack([_video((3, 4, 50, 70), f"metrics.det.a{i}") for i in range(2)]).to(DEV)
    b = torch.stack([_video((3, 4, 50, 70), f"metrics.det.b{i}") for i in range(2)]).to(DEV)
    s1, s2 = metrics.video_stats(a, b), metrics.video_stats(a, b)
    for k in ("sse", "minmax", "ssim_sum"):
        assert torch.equal(s1[k], s2[k]), k
    for i in range(2):
        one = metrics.video_stats(a[i], b[i])
        for k in ("sse", "minmax", "ssim_sum"):
            assert torch.equal(one[k][0], s1[k][i]), (k, i)
    m = metrics.video_metrics(a, b)
    assert m["psnr"].shape == (2, 4) and m["ssim"].shape == (2, 4)
    assert np.array_equal(m["psnr"][1], metrics.video_metrics(a[1], b[1])["psnr"])


def test_mismatched_frame_counts_score_the_common_prefix():
    a, b = _video((3, 6, 16, 24), "metrics.pre.a").to(DEV), _video((3, 4, 16, 24), "metrics.pre.b").to(DEV)
    m = metrics.video_metrics(a, b)
    assert m["psnr"].shape == (4,)
    full = metrics.video_metrics(a[:, :4], b)
    assert np.array_equal(m["psnr"], full["psnr"]) and np.array_equal(m["ssim"], full["ssim"])


def test_refusals():
    x = torch.zeros(3, 2, 6, 32, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.HVKernelError):
        metrics.video_metrics(x, x)                         # H = 6 < the 7x7 window, as skimage raises
    y = torch.zeros(3, 2, 16, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.HVKernelError):
        metrics.video_metrics(y, y)
    z = torch.zeros(3, 2, 16, 32, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.HVKernelError):
        metrics.video_metrics(z.transpose(2, 3), z.transpose(2, 3))      # W not contiguous
    with pytest.raises(_lib.HVKernelError):
        metrics.video_metrics(z.cpu(), z)


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hv_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _read_result(path):
    return dict(ln.split(": ", 1) for ln in open(path).read().split("\n") if ": " in ln)


def test_infer_score_end_to_end_and_study(tmp_path):
    infer = _load_script("infer.py")
    src = tmp_path / "in"
    src.mkdir()
    for i, t in enumerate((5, 9)):                          # fp16-representable inputs: the device's fp16 cast changes nothing
        torch.save(_video((3, t, 32, 48), f"metrics.infer.v{i}").float(), src / f"clip{i}.pt")
    plain = infer.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "plain"), "--reduced"])
    scored = infer.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "scored"), "--reduced", "--score"])
    assert [os.path.basename(p) for p in plain] == [os.path.basename(p) for p in scored] == ["clip0.pt", "clip1.pt"]
    for p, s in zip(plain, scored):
        assert open(p, "rb").read() == open(s, "rb").read()
    assert sorted(os.listdir(tmp_path / "plain")) == ["clip0.pt", "clip1.pt"]
    res = [f for f in os.listdir(tmp_path / "scored") if re.fullmatch(r"metrics_\d{8}_\d{6}\.txt", f)]
    assert len(res) == 1
    got = _read_result(tmp_path / "scored" / res[0])
    assert set(got) == {"Root1", "Root2", "Timestamp", "PSNR", "SSIM"}
    ps, ss = [], []
    for i in range(2):
        x = torch.load(src / f"clip{i}.pt", weights_only=True)
        r = torch.load(tmp_path / "scored" / f"clip{i}.pt", weights_only=True)[0]
        p, s = metrics_ref.video_scores(x.numpy(), r.numpy())
        ps += p.tolist()
        ss += s.tolist()
    assert len(ps) == 14
    print(f"infer --score: PSNR {got['PSNR']} vs {np.mean(ps)}, SSIM {got['SSIM']} vs {np.mean(ss)}")
    assert abs(float(got["PSNR"]) - np.mean(ps)) <= PSNR_TOL and abs(float(got["SSIM"]) - np.mean(ss)) <= SSIM_TOL
    # --no-save: the same numbers, no .pt files; the folder tool scores the saved files to the same result
    infer.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "nosave"), "--reduced", "--score", "--no-save",
                "--results-dir", str(tmp_path / "nosave_res")])
    assert not [f for f in os.listdir(tmp_path / "nosave") if f.endswith(".pt")]
    ns = _read_result(tmp_path / "nosave_res" / os.listdir(tmp_path / "nosave_res")[0])
    assert ns["PSNR"] == got["PSNR"] and ns["SSIM"] == got["SSIM"]
    cm = _load_script("evaluation/compute_metrics.py")
    out = cm.main(["--root1", str(src), "--root2", str(tmp_path / "plain"), "--results-dir", str(tmp_path / "cm")])
    folder = _read_result(out[0])
    assert abs(float(folder["PSNR"]) - np.mean(ps)) <= PSNR_TOL and abs(float(folder["SSIM"]) - np.mean(ss)) <= SSIM_TOL
    # the study driver over the first 3 pooling configurations
    study = _load_script("tools/run_vae_study.py")
    recs = study.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "study"), "--base-config", T_OPS, "--mode", "pool",
                       "--limit", "3", "--reduced"])
    lines = [json.loads(ln) for ln in open(tmp_path / "study" / "study.jsonl")]
    assert len(lines) == 3 == len(recs) and [ln["config"] for ln in lines] == ["exp_1.json", "exp_2.json", "exp_3.json"]
    for ln in lines:
        print(ln)
        if "refused" in ln:
            assert isinstance(ln["refused"], str) and ln["refused"]
        else:
            assert np.isfinite(ln["PSNR"]) and np.isfinite(ln["SSIM"]) and ln["frames"] > 0 and 0 < ln["compression"] <= 1
