"""CPU: the rules of the raw YUV 4:2:0 -> clip path (include/hv_kernels.h hv_yuv420_to_clip, hunyuanvideo_efficiency_amd/dataset.py)
against statements that do not depend on them.  cv2 is not part of this environment, so nothing here executes the fork: the colour
rule is held to the BT.601 float formula over all 2^24 triples and to known answers computed from its constants, the resize to
float64 half-pixel bilinear interpolation."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _abi, _lib, dataset
from tests import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hv_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_colour_rule_within_one_code_of_the_float_formula_over_all_triples():
    """bound 1 code: the float formula's constants have 3-4 digits (1.164 vs 1220542 / 2^20 = 1.16400), so the two differ by rounding
    (0.5) plus a fraction of a code from the constants.  The luma term is clamped at black in both (Y < 16 counts as 16, the rule's
    max(0, Y - 16)): without that clamp the float formula goes 18.6 codes below the rule at Y = 0, which is a statement about footroom
    handling, not about the constants."""
    U, V = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst = 0.0
    for y in range(256):
        Y = np.full_like(U, y)
        r, g, b = yuv_ref.colour(Y, U, V)
        yf = 1.164 * max(0, y - 16)
        fr = np.clip(yf + 1.596 * (V - 128), 0, 255)
        fg = np.clip(yf - 0.813 * (V - 128) - 0.391 * (U - 128), 0, 255)
        fb = np.clip(yf + 2.018 * (U - 128), 0, 255)
        worst = max(worst, float(np.abs(r - fr).max()), float(np.abs(g - fg).max()), float(np.abs(b - fb).max()))
    print(f"largest deviation from the float formula: {worst}")
    assert worst <= 1.0


def test_colour_fits_int32():
    """every sum in front of the shift, at the extremes of its terms (each is monotonic in Y, U and V)"""
    yy, half = (255 - 16) * 1220542, 1 << 19
    hi = max(yy + 1673527 * 127, yy + 852492 * 128 + 409993 * 128, yy + 2116026 * 127) + half
    lo = min(-1673527 * 128, -852492 * 127 - 409993 * 127, -2116026 * 128) + half
    print(f"range in front of the shift: [{lo}, {hi}]")
    assert hi < 2 ** 31 and lo >= -2 ** 31 and 5.5e8 < hi < 5.7e8


KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((128, 128, 128), (130, 130, 130)),
         ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)), ((0, 0, 0), (0, 154, 0)),
         ((255, 255, 255), (255, 125, 255))]


def test_known_answers():
    for (y, u, v), rgb in KNOWN:
        got = tuple(int(c) for c in yuv_ref.colour(np.int64(y), np.int64(u), np.int64(v)))
        assert got == rgb, ((y, u, v), got, rgb)


def _frames(T, W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(T, W * H * 3 // 2), dtype=np.uint8)


def test_layouts_share_pixels():
    """one picture written in the three layouts converts to one RGB frame; pixel (y, x) takes chroma (y >> 1, x >> 1)"""
    W, H = 6, 4
    f = _frames(2, W, H, 0)
    n, q = W * H, W * H // 4
    yv12 = np.concatenate([f[:, :n], f[:, n + q:], f[:, n:n + q]], axis=1)
    nv12 = np.concatenate([f[:, :n], np.stack([f[:, n:n + q], f[:, n + q:]], axis=2).reshape(2, -1)], axis=1)
    a = yuv_ref.rgb_frames(f, W, H, "I420")
    assert np.array_equal(a, yuv_ref.rgb_frames(yv12, W, H, "YV12")) and np.array_equal(a, yuv_ref.rgb_frames(nv12, W, H, "NV12"))
    Y, U, V = yuv_ref.planes(f, W, H, "I420")
    r, g, b = yuv_ref.colour(Y[1, 3, 5], U[1, 1, 2], V[1, 1, 2])
    assert (a[0, 1, 3, 5], a[1, 1, 3, 5], a[2, 1, 3, 5]) == (r, g, b)


def _bilinear_f64(img, OH, OW):
    H, W = img.shape

    def axis(src, dst):
        f = (np.arange(dst) + 0.5) * (src / dst) - 0.5
        f = np.clip(f, 0, src - 1)
        s = np.minimum(np.floor(f).astype(np.int64), src - 1)
        return s, np.minimum(s + 1, src - 1), f - s
    y0, y1, ay = axis(H, OH)
    x0, x1, ax = axis(W, OW)
    top = img[y0][:, x0] * (1 - ax) + img[y0][:, x1] * ax
    bot = img[y1][:, x0] * (1 - ax) + img[y1][:, x1] * ax
    return top * (1 - ay)[:, None] + bot * ay[:, None]


def test_resize_rule():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(10, 14)).astype(np.int64)
    assert yuv_ref.resize(img, 10, 14) is img                      # equal sizes: the identity
    for v in (0, 1, 127, 254, 255):
        assert np.array_equal(yuv_ref.resize(np.full((10, 14), v, dtype=np.int64), 6, 8), np.full((6, 8), v))
        assert np.array_equal(yuv_ref.resize(np.full((6, 8), v, dtype=np.int64), 10, 14), np.full((10, 14), v))
    worst = 0.0
    for (H, W), (OH, OW) in (((10, 14), (6, 8)), ((6, 8), (10, 14)), ((2, 2), (5, 7)), ((1080, 1920), (240, 426))):
        img = rng.integers(0, 256, size=(H, W)).astype(np.int64)
        out = yuv_ref.resize(img, OH, OW)
        assert out.shape == (OH, OW) and out.min() >= 0 and out.max() <= 255
        worst = max(worst, float(np.abs(out - _bilinear_f64(img.astype(np.float64), OH, OW)).max()))
    print(f"largest deviation from float64 bilinear: {worst}")
    assert worst <= 1.0


@pytest.mark.parametrize("src,dst", [(10, 6), (6, 10), (2, 5), (14, 8), (1080, 240), (1920, 426), (64, 1), (96, 2), (7, 7), (1, 3)])
def test_tables(src, dst):
    tab = dataset.resize_tables(src, dst)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (dst, 2)
    s, c1 = tab[:, 0].numpy().astype(np.int64), tab[:, 1].numpy().astype(np.int64)
    i0, i1, c0, r1 = yuv_ref.axis_table(src, dst)
    assert np.array_equal(s, i0) and np.array_equal(c1, r1) and np.array_equal(c0 + c1, np.full(dst, 2048))
    assert s.min() >= 0 and s.max() <= src - 1 and np.minimum(s + 1, src - 1).max() <= src - 1
    assert c1.min() >= 0 and c1.max() <= 2048
    f = (np.arange(dst) + 0.5) * (src / dst) - 0.5
    assert (c1[f < 0] == 0).all() and (c1[f >= src - 1] == 0).all()          # both clamped ends
    if dst > src:
        assert c1[0] == 0 and c1[-1] == 0 and s[0] == 0 and s[-1] == src - 1


def test_target_size():
    assert dataset.target_size(1920, 1080, 240) == (426, 240)
    assert dataset.target_size(1920, 1080, 360) == (640, 360)
    assert dataset.target_size(1920, 1080, 250) == (444, 250)         # 444.4 -> 444
    assert dataset.target_size(854, 480, 270) == (480, 270)           # 480.375 -> 480
    assert dataset.target_size(1000, 600, 125) == (208, 125)          # 208.33 -> 208; and where the halving bites:
    assert dataset.target_size(720, 480, 150) == (224, 150)           # 225 -> 224
    with pytest.raises(ValueError):
        dataset.target_size(1920, 1080, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_value_table_bits(dtype):
    tab = dataset.yuv_value_table(dtype)
    want = torch.stack([((torch.tensor(q, dtype=torch.uint8).float() / 255) * 2 - 1).to(dtype) for q in range(256)])
    assert tab.dtype == dtype and tuple(tab.shape) == (256,)
    it = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(tab.view(it), want.view(it)) and torch.equal(tab.view(it), yuv_ref.value_table(dtype).view(it))
    assert float(tab[0]) == -1.0 and float(tab[255]) == 1.0
    with pytest.raises(_lib.HVKernelError):
        dataset.yuv_value_table(torch.bfloat16)


def test_name_parser():
    assert dataset.parse_yuv_name("flowers-60fps-360-1920x1080.yuv") == (60.0, 1920, 1080)
    assert dataset.parse_yuv_name("a_15fps_120fps_64x32_8x8.yuv") == (15.0, 64, 32)        # first match of each
    for bad in ("flowers-360-1920x1080.yuv", "flowers-60fps.yuv", "clip.yuv"):
        with pytest.raises(ValueError):
            dataset.parse_yuv_name(bad)


def test_frame_range():
    W, H = 8, 4
    fb = W * H * 3 // 2
    fr = dataset.yuv_frame_range
    assert fr(7 * fb, W, H) == (0, 7)
    assert fr(7 * fb, W, H, None, None) == (0, 7)
    assert fr(7 * fb + fb - 1, W, H) == (0, 7)                  # a truncated last frame is dropped
    assert fr(7 * fb, W, H, 2, 5) == (2, 5)
    assert fr(7 * fb, W, H, 2, 100) == (2, 7)                   # end clipped to the whole frames
    assert fr(7 * fb, W, H, None, 3) == (0, 3)
    assert fr(7 * fb, W, H, 3, None) == (3, 7)
    for s, e in ((5, 5), (6, 2), (7, None), (9, 20)):           # start >= end: empty
        a, b = fr(7 * fb, W, H, s, e)
        assert a == b
    assert fr(fb - 1, W, H)[0] == fr(fb - 1, W, H)[1]           # not one whole frame
    for bad in ((7, 4), (8, 3), (0, 4)):
        with pytest.raises(ValueError):
            fr(100, *bad)
    with pytest.raises(ValueError):
        fr(7 * fb, W, H, -1, None)


def test_dataset_lists_and_skips(tmp_path, capsys):
    fb = 8 * 4 * 3 // 2
    (tmp_path / "b_30fps_8x4.yuv").write_bytes(bytes(3 * fb))
    (tmp_path / "a_25fps_8x4.yuv").write_bytes(bytes(2 * fb + 5))
    (tmp_path / "short_30fps_8x4.yuv").write_bytes(bytes(fb - 1))          # no whole frame
    (tmp_path / "noname.yuv").write_bytes(bytes(fb))                        # no size in the name
    (tmp_path / "other.pt").write_bytes(b"")
    ds = dataset.YuvClipDataset(str(tmp_path))
    assert ds.tensor_files == ["a_25fps_8x4.yuv", "b_30fps_8x4.yuv"] and len(ds) == 2
    assert ds.fps == {"a_25fps_8x4.yuv": 25.0, "b_30fps_8x4.yuv": 30.0}
    assert sorted(ds.skipped) == ["noname.yuv", "short_30fps_8x4.yuv"]
    out = capsys.readouterr().out
    assert "Skipping short_30fps_8x4.yuv" in out and "Skipping noname.yuv" in out
    assert len(dataset.YuvClipDataset(str(tmp_path), start=2)) == 1          # only b has a frame 2
    assert dataset.clip_stem("b_30fps_8x4.yuv") == "b_30fps_8x4" and dataset.clip_stem("clip0.pt") == "clip0"


def test_cpu_tensors_are_refused():
    with pytest.raises(_lib.HVKernelError):
        dataset.yuv_to_clip(torch.zeros(8 * 4 * 3 // 2, dtype=torch.uint8), 8, 4)
    with pytest.raises(ValueError):
        dataset.yuv_frame_bytes(7, 4)


def test_infer_arguments():
    infer = _load_script("infer.py")
    base = ["--tensor-dir", "in", "--output-dir", "out"]
    old = infer.parse_args(base + ["--reduced", "--score", "--spectrum", "--fps", "30", "--max-files", "2", "--batch-size", "3"])
    assert (old.tensor_dir, old.output_dir, old.reduced, old.score, old.spectrum, old.fps, old.max_files, old.batch_size, old.vae_path,
            old.config_json, old.no_save, old.results_dir, old.mp4, old.num_workers) == \
        ("in", "out", True, True, True, 30.0, 2, 3, None, None, False, None, False, 4)
    assert (old.yuv_format, old.target_height, old.start_frame, old.end_frame) == (None, None, None, None)
    new = infer.parse_args(base + ["--yuv-format", "NV12", "--target-height", "240", "--start-frame", "3", "--end-frame", "40", "--score",
                                   "--spectrum"])
    assert (new.yuv_format, new.target_height, new.start_frame, new.end_frame, new.fps) == ("NV12", 240, 3, 40, None)
    assert infer.parse_args(base + ["--yuv-format", "I420"]).target_height is None
    for bad in (["--target-height", "240"], ["--start-frame", "1"], ["--end-frame", "9"], ["--yuv-format", "UYVY"],
                ["--yuv-format", "I420", "--target-height", "0"], ["--yuv-format", "I420", "--start-frame", "-1"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + bad)


def test_study_arguments():
    study = _load_script("tools/run_vae_study.py")
    base = ["--tensor-dir", "in", "--output-dir", "out", "--base-config", "c.json"]
    old = study.parse_args(base + ["--mode", "stride", "--limit", "3", "--reduced", "--spectrum", "--fps", "24"])
    assert (old.tensor_dir, old.output_dir, old.base_config, old.config_dir, old.mode, old.limit, old.reduced, old.spectrum, old.fps,
            old.max_files, old.vae_path) == ("in", "out", "c.json", None, "stride", 3, True, True, 24.0, None, None)
    assert (old.yuv_format, old.target_height, old.start_frame, old.end_frame) == (None, None, None, None)
    new = study.parse_args(base + ["--yuv-format", "YV12", "--target-height", "360", "--end-frame", "33", "--spectrum"])
    assert (new.yuv_format, new.target_height, new.start_frame, new.end_frame, new.fps) == ("YV12", 360, None, 33, None)
    for bad in (["--target-height", "240"], ["--start-frame", "1"], ["--end-frame", "9"], ["--yuv-format", "P010"]):
        with pytest.raises(SystemExit):
            study.parse_args(base + bad)


def test_yuv_tensor_arguments():
    tool = _load_script("dataset_processor/yuv_tensor.py")
    base = ["--video-dir", "v", "--output-dir", "o"]
    a = tool.parse_args(base)
    assert (a.video_dir, a.output_dir, a.yuv_format, a.target_height, a.start_frame, a.end_frame) == ("v", "o", "I420", None, None, None)
    a = tool.parse_args(base + ["--target_height", "240", "--start_frame", "2", "--end_frame", "10", "--yuv_format", "NV12"])
    assert (a.yuv_format, a.target_height, a.start_frame, a.end_frame) == ("NV12", 240, 2, 10)
    for bad in (["--yuv_format", "RGB"], ["--target_height", "0"], ["--start_frame", "-2"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    with pytest.raises(SystemExit):
        tool.parse_args(["--video-dir", "v"])


def test_abi_v11_matches_the_header():
    assert _lib.ABI_VERSION == 11
    with open(os.path.join(ROOT, "tests", "golden", "abi_v11.json")) as f:
        rec = json.load(f)
    now = [{"name": name, "returns": ret, "params": [t for t, _ in params]} for ret, name, params in _abi.DECLS]
    assert rec["abi_version"] == 11 and rec["declarations"] == now
    new = [d for d in now if d["name"] == "hv_yuv420_to_clip"]
    assert len(new) == 1 and new[0]["returns"] == "int" and len(new[0]["params"]) == 16
    with open(os.path.join(ROOT, "tests", "golden", "abi_v10.json")) as f:
        old = json.load(f)["declarations"]
    assert [d for d in now if d["name"] != "hv_yuv420_to_clip"] == old          # version 11 only adds
    M = _abi.MACROS
    assert (M["HV_YUV_I420"], M["HV_YUV_YV12"], M["HV_YUV_NV12"], M["HV_YUV_COEF_BITS"]) == (0, 1, 2, 11)
    assert dataset.YUV_FORMATS == {"I420": 0, "YV12": 1, "NV12": 2} and 1 << dataset.COEF_BITS == yuv_ref.COEF
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.hv_abi_version() == 11
        # refusals need no GPU: nothing is launched
        assert lib.hv_yuv420_to_clip(1, 1, 0, 7, 4, 1, 0, 100, 100, 8, 4, 7, None, None, 1, None) == -1
