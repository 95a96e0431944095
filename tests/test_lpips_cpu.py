"""CPU: the host half of the LPIPS scoring - weight loading in its three key layouts, the input LUT against the reference's torch
expression, the float64 restatement tests/lpips_ref.py against a hand-written window-by-window evaluation, result files, the
command-line switches.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _lib, metrics
from hunyuanvideo_efficiency_amd.metrics import LPIPS_CONVS, LpipsAlex, MetricsAccumulator
from tests import lpips_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script(rel):
    spec = importlib.util.spec_from_file_location("hv_lpips_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _state_dicts(model):
    """(torchvision AlexNet state dict with classifier keys, LPIPS linear file, full LPIPS state dict) holding `model`'s weights"""
    alex, lin, full = {}, {}, {}
    for i, ((w, b), v, (idx, *_)) in enumerate(zip(model.convs, model.lins, LPIPS_CONVS)):
        alex[f"features.{idx}.weight"], alex[f"features.{idx}.bias"] = w, b
        full[f"net.slice{i + 1}.{idx}.weight"], full[f"net.slice{i + 1}.{idx}.bias"] = w, b
        lin[f"lin{i}.model.1.weight"] = full[f"lin{i}.model.1.weight"] = v.reshape(1, -1, 1, 1)
    alex["classifier.1.weight"], alex["classifier.1.bias"] = torch.zeros(8, 16), torch.zeros(8)
    full["scaling_layer.shift"], full["scaling_layer.scale"] = torch.zeros(1, 3, 1, 1), torch.ones(1, 3, 1, 1)
    return alex, lin, full


def _same(a, b):
    return all(torch.equal(wa, wb) and torch.equal(ba, bb) for (wa, ba), (wb, bb) in zip(a.convs, b.convs)) and \
        all(torch.equal(x, y) for x, y in zip(a.lins, b.lins))


def test_loader_accepts_the_three_key_layouts_and_names_what_is_missing(tmp_path):
    model = LpipsAlex.synthetic(3)
    alex, lin, full = _state_dicts(model)
    assert _same(LpipsAlex.from_state_dict(alex, lin), model)
    assert _same(LpipsAlex.from_state_dict(full), model)
    torch.save(alex, str(tmp_path / "alexnet.pth"))
    torch.save(lin, str(tmp_path / "alex_lin.pth"))
    torch.save(full, str(tmp_path / "lpips_full.pt"))
    assert _same(LpipsAlex.from_files(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex_lin.pth")), model)
    assert _same(LpipsAlex.from_files(str(tmp_path / "lpips_full.pt")), model)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*lin4\.model\.1\.weight"):
        LpipsAlex.from_state_dict(alex)                                          # the trunk alone
    short = {k: v for k, v in alex.items() if not k.startswith("features.6.")}
    torch.save(short, str(tmp_path / "short.pth"))
    with pytest.raises(ValueError, match=r"features\.6\."):
        LpipsAlex.from_files(str(tmp_path / "short.pth"), str(tmp_path / "alex_lin.pth"))
    bad = dict(alex)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match="layer 2"):
        LpipsAlex.from_state_dict(bad, lin)
    assert _same(LpipsAlex.synthetic(3), model) and not _same(LpipsAlex.synthetic(4), model)


def test_lut_is_the_reference_expression_bit_for_bit():
    """compute_metrics.py:44-60 on a frame holding every byte value, then lpips.py:147-154"""
    lut = metrics.lpips_lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    img = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)           # [1, 256, 3]
    t = torch.from_numpy(img / 255.0).float().permute(2, 0, 1).unsqueeze(0)
    t = t * 2 - 1
    shift = torch.Tensor([-.030, -.088, -.188])[None, :, None, None]
    scale = torch.Tensor([.458, .448, .450])[None, :, None, None]
    want = ((t - shift) / scale)[0, :, 0, :]
    assert t.dtype == torch.float32 and torch.equal(lut.view(torch.int32), want.contiguous().view(torch.int32))
    packed = metrics.lpips_pack_conv(torch.arange(64 * 363, dtype=torch.float32).reshape(64, 3, 11, 11), True)
    assert tuple(packed.shape) == (384, 64) and float(packed[(2 * 11 + 5) * 11 + 7, 9]) == 9 * 363 + 2 * 121 + 5 * 11 + 7
    assert not packed[363:].any()
    w = torch.arange(64 * 32 * 9, dtype=torch.float32).reshape(64, 32, 3, 3)
    assert float(metrics.lpips_pack_conv(w, False)[(1 * 3 + 2) * 32 + 5, 7]) == float(w[7, 5, 1, 2])


def _frames(H, W, key):
    from hunyuanvideo_efficiency_amd import synthetic as syn
    a = syn.hashed_uniform((H, W, 3), key + ".a", 0)
    b = (a + 0.3 * syn.hashed_uniform((H, W, 3), key + ".b", 0)).clamp(-1, 1)
    q = lambda x: ((x + 1) * 127.5).to(torch.uint8).numpy()
    return q(a), q(b)


def test_identical_frames_score_exactly_zero():
    q0, _ = _frames(35, 40, "lpips.cpu.same")
    _, _, layers, total = lpips_ref.frame(q0, q0.copy(), LpipsAlex.synthetic(0))
    assert total == 0.0 and not layers.any()


def _hand_conv(x, w, b, stride, pad):
    """x [C, H, W] float64 numpy, one output pixel at a time"""
    C, H, W = x.shape
    k = w.shape[-1]
    xp = np.zeros((C, H + 2 * pad, W + 2 * pad))
    xp[:, pad:pad + H, pad:pad + W] = x
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = np.empty((w.shape[0], oh, ow))
    for i in range(oh):
        for j in range(ow):
            y[:, i, j] = np.tensordot(w, xp[:, i * stride:i * stride + k, j * stride:j * stride + k], axes=3) + b
    return np.maximum(y, 0.0)


def _hand_pool(x):
    oh, ow = (x.shape[1] - 3) // 2 + 1, (x.shape[2] - 3) // 2 + 1
    return np.array([[x[:, 2 * i:2 * i + 3, 2 * j:2 * j + 3].max(axis=(1, 2)) for j in range(ow)] for i in range(oh)]).transpose(2, 0, 1)


def test_restatement_matches_a_hand_written_31x31_case():
    """31 x 31: maps 7, 3, 1, 1, 1 - taps 3-5 are single pixels"""
    model = LpipsAlex.synthetic(0)
    q0, q1 = _frames(31, 31, "lpips.cpu.hand")
    t0, t1, layers, total = lpips_ref.frame(q0, q1, model)
    assert [tuple(t.shape) for t in t0] == [(1, 64, 7, 7), (1, 192, 3, 3), (1, 384, 1, 1), (1, 256, 1, 1), (1, 256, 1, 1)]
    lut = metrics.lpips_lut().double().numpy()
    feats = []
    for q in (q0, q1):
        x = np.stack([lut[c][q[..., c]] for c in range(3)])
        taps = []
        for i, ((w, b), (_, _, _, _, stride, pad)) in enumerate(zip(model.convs, LPIPS_CONVS)):
            x = _hand_conv(x, w.double().numpy(), b.double().numpy(), stride, pad)
            taps.append(x)
            if i < 2:
                x = _hand_pool(x)
        feats.append(taps)
    want = []
    for a, b, lin, got0 in zip(feats[0], feats[1], model.lins, t0):
        assert np.abs(got0[0].numpy() - a).max() <= 1e-12 * max(1.0, np.abs(a).max())
        na, nb = a / (np.sqrt((a * a).sum(0)) + 1e-10), b / (np.sqrt((b * b).sum(0)) + 1e-10)
        want.append(float(((na - nb) ** 2 * lin.double().numpy()[:, None, None]).sum(0).mean()))
    assert all(v > 0 for v in want)                                              # every tap contributes
    assert np.abs(layers - np.array(want)).max() <= 1e-13 and abs(total - sum(want)) <= 1e-13


def test_accumulator_writes_lpips_only_when_lpips_was_added(tmp_path):
    acc = MetricsAccumulator()
    acc.add([30.0, 40.0], [0.5, 0.6])
    assert list(acc.result()) == ["PSNR", "SSIM"] and "LPIPS" not in open(acc.save(str(tmp_path / "a"), "r1", "r2")).read()
    acc = MetricsAccumulator()
    acc.add([30.0, 40.0, 50.0, 60.0], [0.5, 0.6, 0.7, 0.8], [0.1, 0.2, 0.3, 0.4])    # a 4-frame video
    acc.add([10.0], [0.1], [0.5])                                                    # and a 1-frame one: the mean is over 5 frames
    r = acc.result()
    assert list(r) == ["PSNR", "SSIM", "LPIPS"] and r["LPIPS"] == pytest.approx(0.3, abs=1e-15)
    lines = open(acc.save(str(tmp_path / "b"), "r1", "r2")).read().split("\n")
    assert lines[4:8] == [f"PSNR: {r['PSNR']}", f"SSIM: {r['SSIM']}", f"LPIPS: {r['LPIPS']}", ""]
    with pytest.raises(ValueError):
        acc.add([1.0, 2.0], [0.1, 0.2], [0.5])
    total, layers = metrics.lpips_from_sums(np.array([[49.0, 9.0, 1.0, 2.0, 3.0]]), [49, 9, 1, 1, 1])
    assert total.tolist() == [8.0] and layers.tolist() == [[1.0, 1.0, 1.0, 2.0, 3.0]]


def test_command_line_switches():
    cm, infer, study = _script("evaluation/compute_metrics.py"), _script("infer.py"), _script("tools/run_vae_study.py")
    a = cm.parse_args(["--root1", "p", "--root2", "q", "--results-dir", "r"])
    assert a.lpips_alexnet is None and a.lpips_linear is None
    a = cm.parse_args(["--root1", "p", "--root2", "q", "--results-dir", "r", "--lpips-alexnet", "alexnet.pth", "--lpips-linear", "lin.pth"])
    assert (a.lpips_alexnet, a.lpips_linear) == ("alexnet.pth", "lin.pth")
    with pytest.raises(SystemExit):
        cm.parse_args(["--root1", "p", "--root2", "q", "--results-dir", "r", "--lpips-linear", "lin.pth"])
    with pytest.raises(SystemExit):
        cm.parse_args(["--root1", "p", "--root2", "q", "--results-dir", "r", "--lpips-synthetic"])       # no synthetic mode here
    base = ["--tensor-dir", "d", "--output-dir", "o"]
    a = infer.parse_args(base + ["--score", "--lpips-synthetic"])
    assert a.lpips_synthetic and a.lpips_alexnet is None
    a = infer.parse_args(base + ["--score", "--lpips-alexnet", "full.pt"])
    assert a.lpips_alexnet == "full.pt" and not a.lpips_synthetic
    for bad in (["--lpips-synthetic"], ["--score", "--lpips-synthetic", "--lpips-alexnet", "x"], ["--score", "--lpips-linear", "l"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + bad)
    a = study.parse_args(base + ["--base-config", "c.json", "--lpips-alexnet", "a.pth", "--lpips-linear", "l.pth"])
    assert (a.lpips_alexnet, a.lpips_linear, a.lpips_synthetic) == ("a.pth", "l.pth", False)
    assert study.parse_args(base + ["--config-dir", "c", "--lpips-synthetic"]).lpips_synthetic
    with pytest.raises(SystemExit):
        study.parse_args(base + ["--base-config", "c.json", "--lpips-synthetic", "--lpips-alexnet", "a.pth"])
    assert metrics.lpips_from_args(infer.parse_args(base + ["--score"])) is None
    assert metrics.lpips_from_args(infer.parse_args(base + ["--score", "--lpips-synthetic"])).label == "synthetic"


def test_cpu_tensors_are_refused():
    model = LpipsAlex.synthetic(0)
    x = torch.zeros(3, 2, 32, 32, dtype=torch.float16)
    with pytest.raises(_lib.HVKernelError):
        metrics.lpips_video(x, x, model)
    with pytest.raises(_lib.HVKernelError):
        metrics.video_metrics(x, x, lpips=model)
    with pytest.raises(_lib.HVKernelError):
        MetricsAccumulator(lpips=model).add_video(x, x)
