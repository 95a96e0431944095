"""CPU only: the video tensor -> YUV 4:2:0 rule of include/hv_yuv_write.h as tests/yuv_write_ref.py restates it (known answers, the
BT.601 float formula and the ranges over all 2^24 byte triples, the round trip through the reader's rule), the Y4M header and frame
markers, `.y4m` / `.yuv` name and header parsing with their refusals, and the argument parsing of the three drivers."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from hunyuanvideo_efficiency_amd import _abi, _lib, dataset, video_io
from tests import yuv_ref
from tests import yuv_write_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest |channel error| in codes of RGB -> YUV (this rule) -> RGB (tests/yuv_ref.py:colour, the reader's rule) over all 2^24 byte
# triples on constant 2 x 2 blocks, where both chroma modes give the same sample.  Measured from the two restatements on the CPU; a
# property of the two rules (8-bit limited-range YUV holds fewer colours than 8-bit RGB), not of the kernel.  README "Writing YUV 4:2:0".
ROUND_TRIP_MAX_ERROR = 2


def _load_script(rel):
    spec = importlib.util.spec_from_file_location(os.path.basename(rel)[:-3] + "_yuvw", os.path.join(ROOT, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _triples():
    """all 2^24 byte triples, one R at a time: (R, G, B) int64 [65536]"""
    g, b = (a.reshape(-1) for a in np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij"))
    for r in range(256):
        yield np.full_like(g, r), g, b


@pytest.mark.parametrize("rgb,yuv", [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((255, 0, 0), (82, 90, 240)),
                                     ((0, 255, 0), (145, 54, 34)), ((0, 0, 255), (41, 240, 110))],
                         ids=["black", "white", "red", "green", "blue"])
def test_known_answers(rgb, yuv):
    x = (torch.tensor(rgb, dtype=torch.float32) / 255).reshape(3, 1, 1, 1).expand(3, 2, 4, 6)
    for chroma in ("topleft", "mean"):
        Y, U, V = R.yuv_planes(R.quantise(x, False), chroma)
        assert (Y == yuv[0]).all() and (U == yuv[1]).all() and (V == yuv[2]).all(), (chroma, Y[0, 0, 0], U[0, 0, 0], V[0, 0, 0])
        f = R.frames(x, "I420", False, chroma)
        assert f.shape == (2, 36) and (f[:, :24] == yuv[0]).all() and (f[:, 24:30] == yuv[1]).all() and (f[:, 30:] == yuv[2]).all()
    # [-1, 1] input with rescale gives the same bytes; a gray input is R = G = B
    assert (R.frames(x * 2 - 1, "NV12", True) == R.frames(x, "NV12", False)).all()
    gray = torch.full((1, 1, 2, 2), 0.5)
    assert (R.frames(gray) == R.frames(gray.expand(3, 1, 2, 2))).all()


def test_every_triple_against_the_float_formula_and_the_ranges():
    worst = np.zeros(3)
    for r, g, b in _triples():
        Y = R.luma(r, g, b)
        U, V = R.chroma_uv(r, g, b)
        assert Y.min() >= 16 and Y.max() <= 235 and min(U.min(), V.min()) >= 16 and max(U.max(), V.max()) <= 240
        # the sums of a constant block give the sample of its pixel, and the int32 of the kernel holds every intermediate
        Us, Vs = R.chroma_uv(4 * r, 4 * g, 4 * b, 22)
        assert (Us == U).all() and (Vs == V).all()
        yf = 16 + 0.257 * r + 0.504 * g + 0.098 * b
        uf = 128 - 0.148 * r - 0.291 * g + 0.439 * b
        vf = 128 + 0.439 * r - 0.368 * g - 0.071 * b
        worst = np.maximum(worst, [np.abs(Y - yf).max(), np.abs(U - uf).max(), np.abs(V - vf).max()])
    print("largest |fixed point - float formula| (Y, U, V):", worst)
    assert (worst <= 1).all(), worst
    for s in ((0, 0, 1020), (1020, 0, 0), (0, 1020, 0), (1020, 1020, 1020)):          # the extreme sums of four pixels
        for coef in ((-155188, -305135, 460324), (460324, -385875, -74448)):
            assert abs(sum(c * v for c, v in zip(coef, s))) + (128 << 22) + (1 << 21) < 2 ** 31


def test_mean_chroma_extremes_stay_in_range():
    """blocks mixing the corners of the RGB cube: the sums' samples stay in 16 .. 240"""
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], dtype=np.int64)
    idx = np.stack(np.meshgrid(*[np.arange(8)] * 4, indexing="ij"), -1).reshape(-1, 4)
    s = corners[idx].sum(axis=1)
    U, V = R.chroma_uv(s[:, 0], s[:, 1], s[:, 2], 22)
    assert U.min() >= 16 and U.max() <= 240 and V.min() >= 16 and V.max() <= 240


def test_round_trip_through_the_readers_rule():
    worst = 0
    for r, g, b in _triples():
        Y = R.luma(r, g, b)
        U, V = R.chroma_uv(r, g, b)
        r2, g2, b2 = yuv_ref.colour(Y, U, V)
        worst = max(worst, int(np.abs(r2 - r).max()), int(np.abs(g2 - g).max()), int(np.abs(b2 - b).max()))
    print("largest round-trip channel error:", worst)
    assert worst == ROUND_TRIP_MAX_ERROR


def test_quantiser_is_frames_uint8():
    from hunyuanvideo_efficiency_amd.utils.file_utils import frames_uint8
    for rescale in (False, True):
        k = torch.arange(256, dtype=torch.float32)
        v = torch.cat([k / 255, (k + 0.5) / 255, torch.nextafter(k / 255, torch.tensor(2.0)), torch.nextafter(k / 255, torch.tensor(-2.0)),
                       torch.tensor([-0.25, 1.25, 7.0])])
        v = v * 2 - 1 if rescale else v
        for dtype in (torch.float32, torch.float16):
            x = v.to(dtype).reshape(1, 1, 1, 1, -1).expand(1, 3, 1, 1, -1)
            want = np.stack(frames_uint8(x, rescale))[0, 0, :, 0]
            assert (R.quantise(x[0], rescale)[0, 0, 0] == want).all()
    special = torch.tensor([float("nan"), float("inf"), float("-inf")]).reshape(1, 1, 1, 3)
    assert R.quantise(special, False).reshape(-1).tolist() == [0, 255, 0] and R.quantise(special, True).reshape(-1).tolist() == [0, 255, 0]


def test_layouts():
    x = R.edge_values((3, 2, 4, 6), torch.float32, False, 5)
    Y, U, V = R.yuv_planes(R.quantise(x, False), "mean")
    i420, yv12, nv12 = (R.frames(x, f) for f in ("I420", "YV12", "NV12"))
    assert i420.dtype == np.uint8 and i420.shape == yv12.shape == nv12.shape == (2, 36)
    assert (i420[:, :24] == yv12[:, :24]).all() and (i420[:, :24] == nv12[:, :24]).all() and (i420[:, :24] == Y.reshape(2, -1)).all()
    assert (i420[:, 24:30] == U.reshape(2, -1)).all() and (i420[:, 30:] == V.reshape(2, -1)).all()
    assert (yv12[:, 24:30] == V.reshape(2, -1)).all() and (yv12[:, 30:] == U.reshape(2, -1)).all()
    assert (nv12[:, 24::2] == U.reshape(2, -1)).all() and (nv12[:, 25::2] == V.reshape(2, -1)).all()
    # the reader's plane split is the inverse of the layouts
    for fmt, f in (("I420", i420), ("YV12", yv12), ("NV12", nv12)):
        y, u, v = yuv_ref.planes(f, 6, 4, fmt)
        assert (y == Y).all() and (u == U).all() and (v == V).all()
    # the two chroma modes differ on a block that is not constant and agree on its top-left pixel's formula
    assert (R.frames(x, "I420", chroma="topleft")[:, 24:] != i420[:, 24:]).any()


def test_y4m_header_and_frame_markers():
    assert video_io.y4m_header(1280, 720, 24) == b"YUV4MPEG2 W1280 H720 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert video_io.y4m_header(6, 4, 30000 / 1001) == b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert video_io.y4m_header(6, 4, 29.97).split()[3] == b"F2997:100"
    assert video_io.y4m_header(6, 4, 12.5).split()[3] == b"F25:2"
    for bad in (0, -1, float("nan")):
        with pytest.raises(ValueError):
            video_io.y4m_header(6, 4, bad)
    x = R.edge_values((3, 3, 4, 6), torch.float16, True, 1)
    data = R.y4m_bytes(x, 30000, 1001, rescale=True)
    head = video_io.y4m_header(6, 4, 30000 / 1001)
    assert data.startswith(head) and len(data) == len(head) + 3 * (6 + 36)
    for t in range(3):
        assert data[len(head) + t * 42:len(head) + t * 42 + 6] == dataset.Y4M_FRAME_MARK == b"FRAME\n"
    fps, W, H = dataset.parse_y4m_header(head[:-1])
    assert (W, H) == (6, 4) and abs(fps - 30000 / 1001) < 1e-12


def test_y4m_header_parsing_and_refusals(tmp_path):
    ok = dataset.parse_y4m_header
    assert ok(b"YUV4MPEG2 W8 H4 F25:1") == (25.0, 8, 4)
    assert ok(b"YUV4MPEG2 H4 W8 F30:1 Ip A0:0 C420mpeg2 XYSCSS=420MPEG2") == (30.0, 8, 4)
    assert ok(b"YUV4MPEG2 W8 H4 F60:1 C420paldv") == (60.0, 8, 4) and ok(b"YUV4MPEG2 W8 H4 F60:1 C420") == (60.0, 8, 4)
    for line, token in ((b"YUV4MPEG2 W8 H4 F25:1 C444", "C444"), (b"YUV4MPEG2 W8 H4 F25:1 C422", "C422"),
                        (b"YUV4MPEG2 W8 H4 F25:1 C420p10", "C420p10"), (b"YUV4MPEG2 W8 H4 F25:1 Cmono", "Cmono"),
                        (b"YUV4MPEG2 W8 H4 F25:1 It", "It"), (b"YUV4MPEG2 W8 H4 F25:1 Ib", "Ib"), (b"YUV4MPEG2 W8 H4 F25:1 Im", "Im"),
                        (b"YUV4MPEG2 W8 H4 F25", "F25"), (b"YUV4MPEG2 W8 H4 F25:0", "F25:0"), (b"YUV4MPEG2 Wx H4 F25:1", "Wx")):
        with pytest.raises(ValueError, match=token):
            ok(line)
    for line in (b"YUV4MPEG W8 H4 F25:1", b"YUV4MPEG2 H4 F25:1", b"YUV4MPEG2 W8 F25:1", b"YUV4MPEG2 W8 H4"):
        with pytest.raises(ValueError):
            ok(line)
    # files: the header gives size, rate and the first frame's offset; the dataset lists .y4m beside .yuv and skips what it cannot read
    x = R.edge_values((3, 3, 4, 8), torch.float32, False, 2)
    (tmp_path / "a.y4m").write_bytes(R.y4m_bytes(x, 25, 1))
    (tmp_path / "deep.y4m").write_bytes(b"YUV4MPEG2 W8 H4 F25:1 Ip C420p10\n" + b"FRAME\n" + bytes(96))
    (tmp_path / "b_30fps_8x4.yuv").write_bytes(R.frames(x).tobytes())
    (tmp_path / "nohead.y4m").write_bytes(bytes(2000))
    assert dataset.read_y4m_header(str(tmp_path / "a.y4m")) == (25.0, 8, 4, len(video_io.y4m_header(8, 4, 25)))
    assert dataset.clip_file_info(str(tmp_path / "a.y4m"))[3:] == (len(video_io.y4m_header(8, 4, 25)), 6)
    assert dataset.clip_file_info(str(tmp_path / "b_30fps_8x4.yuv")) == (30.0, 8, 4, 0, 0)
    with pytest.raises(ValueError, match="C420p10"):
        dataset.read_yuv_clip(str(tmp_path / "deep.y4m"), "cpu")
    with pytest.raises(ValueError, match="header"):
        dataset.read_yuv_clip(str(tmp_path / "nohead.y4m"), "cpu")
    with pytest.raises(ValueError, match="I420"):
        dataset.read_yuv_clip(str(tmp_path / "a.y4m"), "cuda", fmt="NV12")
    with pytest.raises(_lib.HVKernelError):                  # CPU devices are refused, after the file has been understood
        dataset.read_yuv_clip(str(tmp_path / "a.y4m"), "cpu")
    ds = dataset.YuvClipDataset(str(tmp_path))
    assert ds.tensor_files == ["a.y4m", "b_30fps_8x4.yuv"] and ds.fps == {"a.y4m": 25.0, "b_30fps_8x4.yuv": 30.0}
    assert sorted(ds.skipped) == ["deep.y4m", "nohead.y4m"]
    assert len(dataset.YuvClipDataset(str(tmp_path), start=3)) == 0 and len(dataset.YuvClipDataset(str(tmp_path), start=2)) == 2
    assert dataset.YuvClipDataset(str(tmp_path), fmt="NV12").tensor_files == ["b_30fps_8x4.yuv"]
    assert dataset.clip_stem("a.y4m") == "a" and dataset.clip_stem("b_30fps_8x4.yuv") == "b_30fps_8x4" and dataset.clip_stem("c.pt") == "c"


def test_yuv_file_names():
    name = video_io.yuv_file_name
    assert name("/o/seed7.yuv", 24, 64, 48) == "/o/seed7_24fps_64x48.yuv"
    assert name("/o/clip_30fps_1920x1080.yuv", 30, 1920, 1080) == "/o/clip_30fps_1920x1080.yuv"           # already right: kept
    assert name("/o/clip_30fps_1920x1080.yuv", 30, 426, 240) == "/o/clip_30fps_426x240.yuv"               # a stale size is replaced
    assert name("clip_60fps_8x4_v2.yuv", 30, 8, 4) == "clip_v2_30fps_8x4.yuv"
    for path, fps, W, H in (("/o/seed7.yuv", 24, 64, 48), ("x_1x1.yuv", 120, 16, 2)):
        assert dataset.parse_yuv_name(os.path.basename(name(path, fps, W, H))) == (float(fps), W, H)
    for bad in (23.976, 0, -24):
        with pytest.raises(ValueError):
            name("a.yuv", bad, 8, 4)


def test_refusals_of_the_python_side(tmp_path):
    x = torch.zeros(3, 2, 4, 8)
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        video_io.clip_to_yuv(x)
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        video_io.write_yuv_clip(x, str(tmp_path / "a.y4m"), 24)
    with pytest.raises(ValueError):
        video_io.clip_to_yuv(x, fmt="UYVY")
    with pytest.raises(ValueError):
        video_io.clip_to_yuv(x, chroma="centre")
    with pytest.raises(ValueError):
        video_io.write_yuv_clip(x, str(tmp_path / "a.mp4"), 24)
    with pytest.raises(ValueError):
        video_io.write_yuv_clip(x, str(tmp_path / "a.y4m"), 24, fmt="NV12")
    assert not os.listdir(tmp_path)
    assert video_io.CHROMA_MODES == {"topleft": 0, "mean": 1} == R.CHROMA
    assert inspect.signature(video_io.clip_to_yuv).parameters["chroma"].default == "mean"
    assert inspect.signature(video_io.write_yuv_clip).parameters["chroma"].default == "mean"


def test_opt_in_defaults():
    from hunyuanvideo_efficiency_amd.diffusion.pipelines import HunyuanVideoPipeline
    from hunyuanvideo_efficiency_amd.utils.file_utils import save_videos_grid
    assert inspect.signature(HunyuanVideoPipeline.__call__).parameters["return_on_device"].default is False
    assert inspect.signature(save_videos_grid).parameters["chroma"].default == "mean"
    assert _abi.MACROS["HV_ABI_VERSION"] == 11


def test_sample_video_arguments(capsys):
    sv = _load_script("sample_video.py")
    a = sv.parse_args([])
    assert (a.save_format, a.save_chroma, a.save_path) == ("auto", None, "./results")
    a = sv.parse_args(["--save-format", "y4m"])
    assert (a.save_format, a.save_chroma) == ("y4m", None)
    a = sv.parse_args(["--save-format", "yuv", "--save-chroma", "topleft"])
    assert (a.save_format, a.save_chroma) == ("yuv", "topleft")
    for bad in (["--save-chroma", "mean"], ["--save-format", "auto", "--save-chroma", "topleft"], ["--save-format", "mp4"],
                ["--save-format", "y4m", "--save-chroma", "centre"]):
        with pytest.raises(SystemExit):
            sv.parse_args(bad)
    assert "--save-chroma is only valid with --save-format" in capsys.readouterr().err


def test_infer_arguments():
    infer = _load_script("infer.py")
    base = ["--tensor-dir", "in", "--output-dir", "out"]
    assert infer.parse_args(base).save_yuv is None
    for choice in ("y4m", "I420", "YV12", "NV12"):
        assert infer.parse_args(base + ["--save-yuv", choice]).save_yuv == choice
    a = infer.parse_args(base + ["--save-yuv", "I420", "--no-save", "--fps", "30"])
    assert (a.save_yuv, a.no_save, a.fps, a.score) == ("I420", True, 30.0, False)
    a = infer.parse_args(base + ["--score", "--no-save", "--save-yuv", "y4m", "--yuv-format", "NV12"])
    assert (a.save_yuv, a.no_save, a.yuv_format) == ("y4m", True, "NV12")
    for bad in (["--save-yuv", "mp4"], ["--save-yuv", "i420"], ["--no-save"], ["--fps", "30"], ["--save-yuv", "I420", "--fps", "0"]):
        with pytest.raises(SystemExit):
            infer.parse_args(base + bad)


def test_study_arguments():
    study = _load_script("tools/run_vae_study.py")
    base = ["--tensor-dir", "in", "--output-dir", "out", "--base-config", "c.json"]
    assert study.parse_args(base).save_yuv is None
    a = study.parse_args(base + ["--save-yuv", "NV12", "--fps", "25"])
    assert (a.save_yuv, a.fps, a.spectrum) == ("NV12", 25.0, False)
    assert "save_yuv" in inspect.signature(study.run_config).parameters
    for bad in (["--save-yuv", "P010"], ["--fps", "25"], ["--save-yuv", "y4m", "--fps", "-1"]):
        with pytest.raises(SystemExit):
            study.parse_args(base + bad)
