"""Gaussian-window SSIM on the GPU (csrc/hv_gssim.hip) against the float64 restatement tests/gssim_ref.py, every [To][C] sum within the
bound tests/gssim_bounds.py derives from the arithmetic include/hv_gssim.h states: through torch.ops.hv and through the C ABI, at every
wrap count of the temporal ring, at every tile edge on both axes, for both dtypes, channel counts, quantiser modes and window forms, on
views whose offsets pass 2^31; the flat-bright sensitivity, locality, determinism, poisoned buffers, one refusal per rule, the Python
entry points, and the driver flags end to end."""
import csv
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _abi, _lib, metrics  # noqa: E402
from tests import gssim_bounds as gb  # noqa: E402
from tests import gssim_ref as ref  # noqa: E402
from tests import metrics_ref  # noqa: E402
from tests.guarded_memory import INT, NAN_BITS  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OPS = os.path.join(ROOT, "tests", "golden", "t_ops_config.json")
_DT = {torch.float16: 0, torch.float32: 1}
PARAMS = {name: params for _, name, params in _abi.GSSIM_DECLS}
WIN, TH, TW = gb.WIN, gb.TILE_H, gb.TILE_W
SENT64 = -7.25e300
W32, W64 = ref.window("fp32"), ref.window("fp64")


def _win(w):
    return torch.from_numpy(np.asarray(w, dtype=np.float64)).to(DEV)


def _values(q, dtype, rescale):
    """codes -> values of `dtype` in the middle of each code's interval, which the quantiser takes back to the code"""
    x = (torch.as_tensor(np.asarray(q), dtype=torch.float64) + 0.5) / 255.0
    return (x * 2.0 - 1.0 if rescale else x).to(dtype)


def _codes(x, rescale):
    """the 8-bit frames of a tensor by the fp32-stepwise quantiser of tests/metrics_ref.py (the kernel's, bit for bit:
    tests/test_gpu_quantiser.py)"""
    return metrics_ref.quantise(x.detach().float().cpu().numpy(), rescale)


def _run(a, b, temporal, rescale, w, ws_fill=None):
    """torch.ops.hv.gaussian_ssim on [C,T,H,W] views; sentinel-guarded output, poisoned workspace -> [To][C] numpy"""
    C, T, H, W = a.shape
    need = _lib.host("gaussian_ssim_workspace_bytes", C, T, H, W, temporal)
    assert need == gb.ntiles(H, W) * (T - 10 * temporal) * C * 8
    To = T - 10 * temporal
    buf = torch.full((4 + To * C + 64,), SENT64, dtype=torch.float64, device=DEV)      # the output between sentinel cells
    out = buf[4:4 + To * C]
    ws = torch.full((need // 8 + 4,), float("nan") if ws_fill is None else ws_fill, dtype=torch.float64, device=DEV)
    _lib.call("gaussian_ssim", a, a.stride(0), a.stride(1), a.stride(2), b, b.stride(0), b.stride(1), b.stride(2), _DT[a.dtype], C, T, H, W,
              rescale, temporal, _win(w), out, ws, need)
    torch.cuda.synchronize()
    assert bool((buf[:4] == SENT64).all()) and bool((buf[4 + To * C:] == SENT64).all()), "cells outside ssim_sum were written"
    assert bool(torch.isnan(ws[need // 8:]).all()) if ws_fill is None else True, "the workspace was written past its size"
    got = out.cpu().numpy().reshape(To, C)
    assert (got != SENT64).all(), "a cell of ssim_sum was not written"
    return got


def _case(shape, temporal, dtype=torch.float16, rescale=1, w=W32, seed=0, kind="noisy"):
    if kind == "noisy":
        qa, qb = gb.noisy_codes(shape, seed)
    elif kind == "random":
        qa, qb = gb.rand_codes(shape, seed), gb.rand_codes(shape, seed + 100)
    elif kind == "near_constant":
        qa, qb = gb.rand_codes(shape, seed, 250, 252), gb.rand_codes(shape, seed + 100, 250, 252)
    elif kind == "identical":
        qa = gb.rand_codes(shape, seed)
        qb = qa
    a, b = _values(qa, dtype, rescale).to(DEV), _values(qb, dtype, rescale).to(DEV)
    assert (_codes(a, rescale) == qa).all() and (_codes(b, rescale) == qb).all()
    got = _run(a, b, temporal, rescale, w)
    return gb.check_sums(got, qa, qb, w, bool(temporal), f"{shape} temporal={temporal} {dtype} rescale={rescale} {kind}"), got


# T: the ring of 11 frames wraps zero, one, two and three times while one workgroup walks the clip - (3, T, 58, 490) has 3 * 45 tiles, from
# which on the kernel walks all frames in one run; the small shapes below split the walk into runs of at least 4 frames
@pytest.mark.parametrize("T", [11, 12, 21, 22, 23, 34])
def test_temporal_ring_in_one_run(T):
    assert 3 * gb.ntiles(58, 490) >= 128
    _case((3, T, 58, 490), 1, seed=T)


# T < 11 only without the temporal window (with it such a clip is refused: test_refusals_leave_the_outputs_untouched)
@pytest.mark.parametrize("T,temporal", [(T, t) for T in (1, 10, 11, 12, 21, 22, 23, 34) for t in (0, 1) if T >= WIN or not t])
def test_frame_counts_on_split_walks(T, temporal):
    _case((1, T, 13, 14), temporal, seed=T, w=W32 if temporal else W64)
    _case((3, T, 12, 11 + TW + 1), temporal, seed=T + 50, kind="random")


# one case per tile edge on each axis (frame extents and map extents around the tile), then edges on both axes at once
H_EDGES = [11, 12, TH - 1, TH, TH + 1, TH + WIN - 2, TH + WIN - 1, TH + WIN, 27, 45]
W_EDGES = [11, 12, TW - 1, TW, TW + 1, TW + WIN - 2, TW + WIN - 1, TW + WIN, 27, 45]


@pytest.mark.parametrize("H", H_EDGES)
def test_tile_edges_along_h(H):
    _case((1, 11, H, 12), 1, seed=H)
    _case((1, 2, H, 12), 0, seed=H + 1, w=W64)


@pytest.mark.parametrize("W", W_EDGES)
def test_tile_edges_along_w(W):
    _case((1, 11, 12, W), 1, seed=W)
    _case((1, 2, 12, W), 0, seed=W + 1, w=W64)


@pytest.mark.parametrize("shape,temporal", [((3, 12, TH + WIN, TW + WIN), 1), ((1, 11, TH + WIN - 1, TW + WIN - 1), 1), ((3, 12, 45, 45), 1),
                                            ((3, 2, 2 * TH + WIN, 2 * TW + WIN), 0), ((1, 3, 27, 45), 0)])
def test_tile_edges_on_both_axes(shape, temporal):
    _case(shape, temporal, seed=sum(shape))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("rescale", [0, 1])
def test_channels_dtypes_and_quantiser_modes(C, dtype, rescale):
    _case((C, 12, 20, 37), 1, dtype, rescale, seed=C + rescale)
    _case((C, 3, 20, 37), 0, dtype, rescale, W64, seed=C + rescale + 7)


@pytest.mark.parametrize("kind", ["random", "near_constant", "identical"])
@pytest.mark.parametrize("form", ["fp32", "fp64"])
def test_input_classes_and_window_forms(kind, form):
    w = ref.window(form)
    ratio, got = _case((3, 13, 24, 40), 1, w=w, kind=kind, seed=3)
    _case((3, 2, 24, 40), 0, w=w, kind=kind, seed=4)
    if kind == "identical":
        assert np.abs(got / (14 * 30) - 1.0).max() < 1e-12


def test_clipped_and_unquantised_inputs():
    """values beyond the quantiser's range on both sides, NaN included, against the quantiser's own bytes"""
    g = torch.Generator().manual_seed(5)
    for dtype, rescale in ((torch.float16, 1), (torch.float32, 0)):
        a = (torch.rand((3, 12, 19, 35), generator=g) * 3.0 - 1.5).to(dtype)
        b = (a.float() + 0.2 * torch.randn(a.shape, generator=g)).to(dtype)
        b[0, 3, 4, 5] = float("nan")
        b[1, 0, 0, 0], b[2, 11, 18, 34] = float("inf"), -float("inf")
        qa, qb = _codes(a, rescale), _codes(torch.nan_to_num(b.float(), nan=-10.0), rescale)     # NaN quantises to 0 (hv_common.hpp)
        assert qa.min() == 0 and qa.max() == 255 and qb[0, 3, 4, 5] == 0
        for temporal in (0, 1):
            gb.check_sums(_run(a.to(DEV), b.to(DEV), temporal, rescale, W32), qa, qb, W32, bool(temporal), f"clipped {dtype}")


def test_flat_bright_sensitivity():
    """codes 250 against one pixel at 251: the kernel's frame means differ by the restatement's difference (1.8e-5), within the bound"""
    qa, qb = gb.flat_pair()
    a, b = _values(qa, torch.float16, 1).to(DEV), _values(qb, torch.float16, 1).to(DEV)
    same, moved = _run(a, a, 1, 1, W32), _run(a, b, 1, 1, W32)
    gb.check_sums(same, qa, qa, W32, True, "flat"), gb.check_sums(moved, qa, qb, W32, True, "flat + 1")
    npos = 14 * 14
    want = (ref.sums(qa, qa, W32, True) - ref.sums(qa, qb, W32, True)) / npos
    bound = (gb.sum_bound(qa, qa, W32, True) + gb.sum_bound(qa, qb, W32, True)) / npos
    got = (same - moved) / npos
    assert (want > 1.8e-5).all() and (bound < 0.5 * want).all()
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)


def _layout(x, kind):
    """x [C,T,H,W] on the device -> a view with the same values inside NaN-filled memory"""
    C, T, H, W = x.shape
    nan, it = NAN_BITS[x.element_size()], INT[x.element_size()]
    if kind == "sliced_h":                   # every other row of a taller, wider buffer
        buf = torch.full((C, T, 2 * H + 1, W + 8), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, :, 1:2 * H:2, 3:3 + W]
    elif kind == "strided_t":                # every third frame
        buf = torch.full((C, 3 * T, H, W), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, 1::3]
    elif kind == "permuted":                 # stored [T, C, H, W]: sc < st
        buf = torch.full((T, C, H, W), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf.permute(1, 0, 2, 3)
    v.copy_(x)
    return v


@pytest.mark.parametrize("kind", ["sliced_h", "strided_t", "permuted"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_views(kind, dtype):
    shape = (3, 12, 18, 36)
    qa, qb = gb.noisy_codes(shape, 31)
    a, b = _layout(_values(qa, dtype, 1).to(DEV), kind), _values(qb, dtype, 1).to(DEV)
    assert not a.is_contiguous()
    for temporal in (0, 1):
        gb.check_sums(_run(a, b, temporal, 1, W32), qa, qb, W32, bool(temporal), kind)
        gb.check_sums(_run(b, a, temporal, 1, W32), qb, qa, W32, bool(temporal), kind + " swapped")


def test_batch_and_frame_count_rule():
    """[B,C,T,H,W] scores video by video; the first min(T_ref, T_rec) frames count"""
    qa, qb = gb.noisy_codes((2, 3, 13, 16, 20), 41)
    a, b = _values(qa, torch.float16, 1).to(DEV), _values(qb, torch.float16, 1).to(DEV)
    s = metrics.gaussian_ssim_sums(a, b[:, :, :12], True, True, _win(W32))
    assert s.shape == (2, 2, 3)
    for i in range(2):
        gb.check_sums(s[i].cpu().numpy(), qa[i][:, :12], qb[i][:, :12], W32, True, f"batch {i}")
    s0 = metrics.gaussian_ssim_sums(a[1], b[1], False, True)           # default window without the temporal axis: the fp64 form
    gb.check_sums(s0[0].cpu().numpy(), qa[1], qb[1], W64, False, "unbatched")


def test_element_offsets_beyond_2_to_31():
    """frames 2^31 + 8 elements apart in an uninitialised buffer of which only the addressed frames are written"""
    H, W, st = 14, 40, (1 << 31) + 8
    qa, qb = gb.noisy_codes((1, 2, H, W), 51)
    views = []
    for q in (qa, qb):
        buf = torch.empty(st + H * W, dtype=torch.float16, device=DEV)
        v = buf.as_strided((1, 2, H, W), (0, st, W, 1))
        v.copy_(_values(q, torch.float16, 1))
        views.append(v)
    gb.check_sums(_run(views[0], views[1], 0, 1, W64), qa, qb, W64, False, "2^31")
    del views, buf
    torch.cuda.empty_cache()


def test_frame_locality_and_determinism():
    """row t depends on frames t .. t + 10 only (on frame t alone without the temporal window); two runs give the same bits, whatever the
    workspace held"""
    shape = (3, 24, 20, 37)
    qa, qb = gb.noisy_codes(shape, 61)
    a, b = _values(qa, torch.float16, 1).to(DEV), _values(qb, torch.float16, 1).to(DEV)
    full = _run(a, b, 1, 1, W32)
    assert (_run(a, b, 1, 1, W32, ws_fill=1.0e300).view(np.int64) == full.view(np.int64)).all()
    b2 = b.clone()
    b2[:, 16] = _values(255 - qb[:, 16], torch.float16, 1).to(DEV)
    moved = _run(a, b2, 1, 1, W32)
    touched = np.array([6 <= t <= 16 for t in range(14)])
    assert (moved[~touched].view(np.int64) == full[~touched].view(np.int64)).all() and (moved[touched] != full[touched]).all()
    head = _run(a[:, :15], b[:, :15], 1, 1, W32)                      # a shorter clip: other runs of the walk, the same rows
    assert (head.view(np.int64) == full[:5].view(np.int64)).all()
    f0, f2 = _run(a, b, 0, 1, W64), _run(a, b2, 0, 1, W64)
    only = np.arange(24) == 16
    assert (f0[~only].view(np.int64) == f2[~only].view(np.int64)).all() and (f0[only] != f2[only]).all()


def test_through_the_c_abi():
    lib = _lib.load()
    shape = (3, 12, 27, 45)
    qa, qb = gb.noisy_codes(shape, 71)
    a, b = _values(qa, torch.float32, 0).to(DEV), _values(qb, torch.float32, 0).to(DEV)
    for temporal, w in ((1, W32), (0, W64)):
        need = lib.hv_gaussian_ssim_workspace_bytes(3, 12, 27, 45, temporal)
        assert need == _lib.host("gaussian_ssim_workspace_bytes", 3, 12, 27, 45, temporal) > 0
        To = 12 - 10 * temporal
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        out = torch.full((To, 3), SENT64, dtype=torch.float64, device=DEV)
        kw = dict(a=a, a_sc=a.stride(0), a_st=a.stride(1), a_sh=a.stride(2), b=b, b_sc=b.stride(0), b_st=b.stride(1), b_sh=b.stride(2),
                  dtype=1, C=3, T=12, H=27, W=45, rescale=0, temporal=temporal, win=_win(w), ssim_sum=out, workspace=ws, workspace_bytes=need)
        args = [None if t == "hipStream_t" else (kw[p].data_ptr() if isinstance(kw[p], torch.Tensor) else kw[p]) for t, p in PARAMS["hv_gaussian_ssim"]]
        torch.cuda.synchronize()
        assert lib.hv_gaussian_ssim(*args) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        gb.check_sums(got, qa, qb, w, bool(temporal), "C ABI")
        assert (got.view(np.int64) == _run(a, b, temporal, 0, w).view(np.int64)).all()        # the op and the C ABI: one kernel


def test_refusals_leave_the_outputs_untouched():
    """one refusal per rule of the header"""
    C, T, H, W = 3, 12, 16, 20
    a = torch.zeros(C, T, H, W, dtype=torch.float16, device=DEV)
    need = _lib.host("gaussian_ssim_workspace_bytes", C, T, H, W, 1)
    out = torch.full((T * C + 1,), SENT64, dtype=torch.float64, device=DEV)
    ws = torch.full((need // 8 + 1,), SENT64, dtype=torch.float64, device=DEV)
    win = _win(W32)
    base = dict(a=a, a_sc=a.stride(0), a_st=a.stride(1), a_sh=a.stride(2), b=a, b_sc=a.stride(0), b_st=a.stride(1), b_sh=a.stride(2), dtype=0,
                C=C, T=T, H=H, W=W, rescale=1, temporal=1, win=win, ssim_sum=out, workspace=ws, workspace_bytes=need)
    order = [p for t, p in PARAMS["hv_gaussian_ssim"] if t != "hipStream_t"]
    _lib.call("gaussian_ssim", *[base[p] for p in order])              # the baseline is accepted
    torch.cuda.synchronize()
    out.fill_(SENT64), ws.fill_(SENT64)
    rules = [dict(H=10), dict(W=10), dict(H=65537), dict(W=65537, a_sh=65537, b_sh=65537), dict(C=2), dict(C=4), dict(T=0, temporal=0),
             dict(T=65536), dict(T=10), dict(dtype=2), dict(rescale=2), dict(temporal=2), dict(a_sc=-1), dict(b_st=-1), dict(a_sh=W - 1),
             dict(b_sh=0), dict(win=None), dict(ssim_sum=None), dict(a=None), dict(b=None), dict(workspace=None),
             dict(win=torch.zeros(23, dtype=torch.float32, device=DEV)[1:]), dict(ssim_sum=out.view(torch.float32)[1:]),
             dict(workspace=ws.view(torch.float32)[1:]), dict(workspace_bytes=need - 1)]
    for ov in rules:
        with pytest.raises(_lib.HVKernelError, match="bad argument|needs at least"):
            _lib.call("gaussian_ssim", *[dict(base, **ov)[p] for p in order])
    torch.cuda.synchronize()
    assert bool((out == SENT64).all()) and bool((ws == SENT64).all())
    q = lambda *s: _lib.host("gaussian_ssim_workspace_bytes", *s)     # noqa: E731
    assert q(2, 12, 16, 20, 1) == q(3, 10, 16, 20, 1) == q(3, 12, 10, 20, 0) == q(3, 12, 16, 65537, 0) == q(3, 0, 16, 20, 0) == 0


def test_python_entry_points_against_the_restatement():
    qa, qb = gb.noisy_codes((3, 14, 22, 38), 81)
    a, b = _values(qa, torch.float16, 1).to(DEV), _values(qb, torch.float16, 1).to(DEV)
    npos = 12 * 28
    tol3 = gb.sum_bound(qa, qb, W32, True).max() / npos + 4 * gb.U       # means of sums within the bound, a few roundings on the host
    tol2 = gb.sum_bound(qa, qb, W64, False).max() / npos + 4 * gb.U
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        g = metrics.gaussian_ssim(a, b)
        m = metrics.video_metrics(a, b, gssim=True)
    assert not [c for c in caught if "T axis" in str(c.message)]               # 14 frames: the window spans T, nothing to warn about
    plain = metrics.video_metrics(a, b)
    assert set(m) == set(plain) | {"ssim3d", "ssim2d", "ssim2d_frames", "temporal"}
    assert all(np.array_equal(m[k], plain[k]) for k in plain)                  # the other scores are what they were
    for d in (g, m):
        assert d["temporal"] is True and isinstance(d["ssim3d"], float) and d["ssim2d_frames"].shape == (14,)
        assert abs(d["ssim3d"] - ref.ssim3d(qa, qb)) <= tol3 and abs(d["ssim2d"] - ref.ssim2d(qa, qb)) <= tol2
        assert np.abs(d["ssim2d_frames"] - ref.ssim2d_frames(qa, qb)).max() <= tol2
    gB = metrics.gaussian_ssim(torch.stack([a, b]), torch.stack([b, b]))
    assert gB["ssim3d"].shape == (2,) and gB["ssim2d_frames"].shape == (2, 14)
    assert abs(gB["ssim3d"][0] - g["ssim3d"]) == 0 and abs(gB["ssim3d"][1] - 1.0) < 1e-12 and abs(gB["ssim2d"][1] - 1.0) < 1e-12
    acc = metrics.MetricsAccumulator(gssim=True)
    acc.add_video(a, b), acc.add_video(b, b)
    res = acc.result()
    assert list(res) == ["PSNR", "SSIM", "SSIM3D", "SSIM2D"]
    assert abs(res["SSIM3D"] - (g["ssim3d"] + gB["ssim3d"][1]) / 2) < 1e-15 and abs(res["SSIM2D"] - (g["ssim2d"] + gB["ssim2d"][1]) / 2) < 1e-15
    off = metrics.MetricsAccumulator()
    off.add_video(a, b)
    assert list(off.result()) == ["PSNR", "SSIM"]


def test_fewer_frames_than_the_window_warn_and_skip_the_axis():
    qa, qb = gb.noisy_codes((3, 5, 16, 17), 91)
    a, b = _values(qa, torch.float16, 1).to(DEV), _values(qb, torch.float16, 1).to(DEV)
    with pytest.warns(UserWarning, match="skips the T axis"):
        g = metrics.gaussian_ssim(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ref.ssim3d(qa, qb)
    assert g["temporal"] is False and abs(g["ssim3d"] - want) <= gb.sum_bound(qa, qb, W32, False).max() / 42 + 4 * gb.U
    with pytest.raises(_lib.HVKernelError, match="refused"):
        metrics.gaussian_ssim_sums(a, b, True)


def test_cpu_tensors_and_bad_windows_are_refused():
    a = torch.zeros(3, 12, 16, 16, dtype=torch.float16)
    for fn in (lambda: metrics.gaussian_ssim(a, a), lambda: metrics.gaussian_ssim_sums(a.to(DEV), a), lambda: metrics.video_metrics(a, a, gssim=True)):
        with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
            fn()
    with pytest.raises(_lib.HVKernelError, match="win"):
        metrics.gaussian_ssim_sums(a.to(DEV), a.to(DEV), True, True, torch.from_numpy(W32))


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hv_gssim_gpu_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _result_lines(d):
    files = [f for f in os.listdir(d) if f.startswith("metrics_") and f.endswith(".txt")]
    assert len(files) == 1
    return [ln.split(":")[0] for ln in open(os.path.join(d, files[0])).read().splitlines() if ln], open(os.path.join(d, files[0])).read()


def test_driver_flags_end_to_end(tmp_path, capsys):
    """a two-clip directory through evaluation/compute_metrics.py, infer.py --score and tools/run_vae_study.py: the CSV rows and result
    lines with the flags, and without them exactly the lines, keys and files the drivers write today"""
    shape = (3, 13, 32, 32)
    src, dst = tmp_path / "in", tmp_path / "rec"
    src.mkdir(), dst.mkdir()
    codes = {}
    for i, name in enumerate(("busy", "calm")):
        qa, qb = gb.noisy_codes(shape, 100 + i, amp=4 + 20 * i)
        codes[name] = (qa, qb)
        torch.save(_values(qa, torch.float16, 1), src / f"{name}.pt")
        torch.save(_values(qb, torch.float16, 1), dst / f"{name}.pt")
    npos = 22 * 22

    # evaluation/compute_metrics.py
    cm = _load_script("evaluation/compute_metrics.py")
    cm.main(["--root1", str(src), "--root2", str(dst), "--results-dir", str(tmp_path / "r0")])
    plain_out = capsys.readouterr().out
    cm.main(["--root1", str(src), "--root2", str(dst), "--results-dir", str(tmp_path / "r1"), "--gssim", "--metrics-csv", str(tmp_path / "r1" / "rows.csv")])
    flag_out = capsys.readouterr().out
    keys0, text0 = _result_lines(tmp_path / "r0")
    keys1, text1 = _result_lines(tmp_path / "r1")
    assert keys0 == ["Root1", "Root2", "Timestamp", "PSNR", "SSIM"]                    # today's lines, nothing else
    assert keys1 == keys0 + ["SSIM3D", "SSIM2D"]
    assert [ln for ln in text1.splitlines() if ln.startswith(("PSNR", "SSIM:"))] == [ln for ln in text0.splitlines() if ln.startswith(("PSNR", "SSIM:"))]
    assert "SSIM3D" not in plain_out and "SSIM2D" not in plain_out
    assert [f for f in _tree(tmp_path / "r0") if not f.startswith("metrics_")] == []
    for name in codes:
        line0 = [ln for ln in plain_out.splitlines() if ln.startswith(name)][0]
        line1 = [ln for ln in flag_out.splitlines() if ln.startswith(name)][0]
        assert line0 == f"{name}.pt: " + line0.split(": ", 1)[1] and " SSIM3D " in line1 and line1.replace(line1[line1.index(" SSIM3D"):line1.index(" (")], "") == line0
    rows = list(csv.reader(open(tmp_path / "r1" / "rows.csv", newline="")))
    assert rows[0] == ["video_path", "ssim", "psnr", "lpips", "fvd", "fvdm"] == metrics.METRICS_CSV_HEADER and len(rows) == 3
    want3 = {}
    for row, name in zip(rows[1:], ("busy", "calm")):
        qa, qb = codes[name]
        assert row[0] == os.path.abspath(dst / f"{name}.pt") and row[3:] == ["", "", ""]
        want3[name] = ref.ssim3d(qa, qb)
        assert abs(float(row[1]) - want3[name]) <= gb.sum_bound(qa, qb, W32, True).max() / npos + 4 * gb.U
        want_psnr = np.mean([metrics_ref.psnr(qa[:, t].transpose(1, 2, 0), qb[:, t].transpose(1, 2, 0)) for t in range(13)])
        assert abs(float(row[2]) - want_psnr) < 1e-9
    val = {ln.split(": ")[0]: ln.split(": ")[1] for ln in text1.splitlines() if ": " in ln}
    assert abs(float(val["SSIM3D"]) - np.mean(list(want3.values()))) < 1e-9
    assert abs(float(val["SSIM2D"]) - np.mean([ref.ssim2d(*codes[n]) for n in codes])) < 1e-9

    # infer.py --score
    infer = _load_script("infer.py")
    base = ["--tensor-dir", str(src), "--reduced", "--config-json", T_OPS, "--score"]
    infer.main(base + ["--output-dir", str(tmp_path / "i0")])
    out0 = capsys.readouterr().out
    infer.main(base + ["--output-dir", str(tmp_path / "i1"), "--gssim", "--metrics-csv", str(tmp_path / "i1.csv")])
    out1 = capsys.readouterr().out
    names = lambda d: [f for f in _tree(d) if not f.startswith("metrics_")]      # noqa: E731
    assert names(tmp_path / "i0") == names(tmp_path / "i1") == ["busy.pt", "calm.pt"]
    for f in ("busy.pt", "calm.pt"):
        assert open(tmp_path / "i0" / f, "rb").read() == open(tmp_path / "i1" / f, "rb").read()
    k0, t0 = _result_lines(tmp_path / "i0")
    k1, t1 = _result_lines(tmp_path / "i1")
    assert k0 == ["Root1", "Root2", "Timestamp", "PSNR", "SSIM"] and k1 == k0 + ["SSIM3D", "SSIM2D"] and "SSIM3D" not in out0
    score0 = [ln for ln in out0.splitlines() if ln.startswith("Scored")]
    score1 = [ln for ln in out1.splitlines() if ln.startswith("Scored")]
    assert len(score0) == 2 and all(" SSIM3D " in ln for ln in score1)
    assert [ln[:ln.index(" SSIM3D")] + ln[ln.index(" ("):] for ln in score1] == score0
    rows = list(csv.reader(open(tmp_path / "i1.csv", newline="")))
    assert rows[0] == metrics.METRICS_CSV_HEADER and [r[0] for r in rows[1:]] == [os.path.abspath(tmp_path / "i1" / f) for f in ("busy.pt", "calm.pt")]
    for r, name in zip(rows[1:], ("busy", "calm")):
        rec = torch.load(tmp_path / "i1" / f"{name}.pt", weights_only=True)[0]
        Tc = min(13, rec.shape[1])
        if Tc >= WIN:                                    # the reconstruction as the scorer saw it (fp16, on the device)
            qa = codes[name][0][:, :Tc]
            g = metrics.gaussian_ssim(_values(qa, torch.float16, 1).to(DEV), rec[:, :Tc].to(DEV, torch.float16))
            assert abs(float(r[1]) - g["ssim3d"]) < 1e-12
        assert 0.0 < float(r[1]) <= 1.0 and float(r[2]) > 0 and r[3:] == ["", "", ""]
    with pytest.raises(SystemExit):
        infer.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "i2"), "--gssim"])       # only with --score
    capsys.readouterr()

    # tools/run_vae_study.py
    study = _load_script("tools/run_vae_study.py")
    common = ["--tensor-dir", str(src), "--base-config", T_OPS, "--mode", "pool", "--limit", "2", "--reduced"]
    plain = study.main(common + ["--output-dir", str(tmp_path / "s0")])
    flagged = study.main(common + ["--output-dir", str(tmp_path / "s1"), "--gssim"])
    assert _tree(tmp_path / "s0") == _tree(tmp_path / "s1")
    seen = 0
    for pl, fl in zip(plain, flagged):
        if "refused" in pl:
            assert fl == pl
            continue
        seen += 1
        assert set(pl) == {"config", "PSNR", "SSIM", "frames", "compression"}                  # today's keys, nothing else
        assert set(fl) == set(pl) | {"ssim3d", "ssim2d"} and all(fl[k] == pl[k] for k in pl)
        assert 0.0 < fl["ssim3d"] <= 1.0 and 0.0 < fl["ssim2d"] <= 1.0
    assert seen >= 1
    assert [json.loads(ln) for ln in open(tmp_path / "s1" / "study.jsonl")] == flagged
