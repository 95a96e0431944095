"""Content histograms and their entropies on the GPU (csrc/hv_content.hip) against the numpy restatement tests/content_ref.py: counts
bit for bit through metrics.content_histograms, torch.ops.hv and the C ABI at every partition edge of the kernel, guarded outputs, slice
invariance, the entropy finaliser within 1e-10 bit of float64 (content_ref.ENTROPY_TOL has the derivation), metrics.content_entropy
field by field, and the driver flags end to end."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _abi, _lib, metrics  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import content_ref as ref  # noqa: E402
from tests.guarded_memory import INT, NAN_BITS, GuardedFlat, poisoned_vec  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OPS = os.path.join(ROOT, "tests", "golden", "t_ops_config.json")
_DT = {torch.float16: 0, torch.float32: 1}
PARAMS = {name: params for _, name, params in _abi.CONTENT_DECLS}
CHUNK = metrics.CONTENT_CHUNK               # pixels of one workgroup (HV_CONTENT_CHUNK)
# the kernel's smaller partitions (csrc/hv_content.hip: kQuad, 64 * kQuad, kThreads * kQuad): a thread takes 4 consecutive pixels, a wave
# 256, one pass of the 256-thread workgroup 1024; a chunk is 8 passes
PER_THREAD, PER_WAVE, PER_PASS = 4, 256, 1024
SENT64 = -7.25e300


def _data(shape, key, dtype=torch.float16, rescale=True):
    """host float32 values that `dtype` holds exactly, a little beyond the quantiser's range on both sides"""
    x = syn.hashed_uniform(shape, key, 0)
    x = 1.1 * x / x.abs().max()
    if not rescale:
        x = x.abs() * 1.05 - 0.02
    return x.to(dtype).float()


def _bytes_clip(q, dtype=torch.float16):
    """bytes [T, H, W] -> [3, T, H, W] in [-1, 1] whose gray frames are q exactly"""
    x = ((torch.as_tensor(np.asarray(q), dtype=torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(dtype)
    return x[None].expand(3, *x.shape).contiguous().float()


def _layout(x, kind):
    """x [3,T,H,W] on the device -> a view with the same values inside NaN-filled memory"""
    C, T, H, W = x.shape
    nan, it = NAN_BITS[x.element_size()], INT[x.element_size()]
    if kind == "contiguous":
        return poisoned_vec(x.contiguous().reshape(-1)).view(C, T, H, W)
    if kind == "rows":                       # row stride above W, every other row of a taller buffer
        buf = torch.full((C, T, 2 * H + 1, W + 8), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, :, 1:2 * H:2, 4:4 + W]
    elif kind == "offset1":                  # the view starts one element into a row: no vector load is aligned
        buf = torch.full((C, T, H, W + 4), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, :, :, 1:1 + W]
    elif kind == "permuted":                 # stored [T, C, H, W]: sc < st
        buf = torch.full((T, C, H, W), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf.permute(1, 0, 2, 3)
    elif kind == "frames":                   # every other frame of a longer buffer
        buf = torch.full((C, 2 * T, H, W), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, ::2]
    else:
        raise ValueError(kind)
    v.copy_(x)
    return v


def _launch(x, rescale=True, luma=metrics.GRAY_LUMA, T=None, strides=None, ws_bytes=None, inter_none=False):
    """one call through torch.ops.hv with guarded outputs and a guarded workspace -> (intra, inter) int64 numpy"""
    _, Tx, H, W = x.shape
    T = Tx if T is None else T
    need = _lib.host("content_histograms_workspace_bytes", T, H, W)
    ws_bytes = need if ws_bytes is None else ws_bytes
    words = max(ws_bytes, 4) // 4
    ws = GuardedFlat(words, torch.int32)
    intra, inter = GuardedFlat(max(T, 1) * 256, torch.int32), GuardedFlat(max(T - 1, 1) * 511, torch.int32)
    sc, st, sh = (x.stride(0), x.stride(1), x.stride(2)) if strides is None else strides
    before = [g.buf.clone() for g in (intra, inter, ws)]
    try:
        _lib.call("content_histograms", x, sc, st, sh, _DT[x.dtype], T, H, W, 1 if rescale else 0, *luma, intra.view,
                  None if inter_none else inter.view, ws.view, ws_bytes)
    except _lib.HVKernelError:
        torch.cuda.synchronize()
        assert all(torch.equal(g.buf, b) for g, b in zip((intra, inter, ws), before)), "a refused call wrote to its outputs or workspace"
        raise
    torch.cuda.synchronize()
    assert intra.intact() and inter.intact() and ws.intact(), "a write outside [T][256], [T-1][511] or the workspace"
    if T == 1:
        assert torch.equal(inter.buf, before[1]), "T = 1 wrote to inter"
    return (intra.view.cpu().numpy().astype(np.int64).reshape(T, 256),
            inter.view.cpu().numpy().astype(np.int64)[:(T - 1) * 511].reshape(T - 1, 511))


def _check(x_host, dtype=torch.float16, layout="contiguous", rescale=True, luma=metrics.GRAY_LUMA, what=""):
    x_dev = x_host.to(DEV, dtype)
    want_i, want_p = ref.histograms(x_dev.float().cpu().numpy(), rescale, luma)
    got_i, got_p = _launch(_layout(x_dev, layout), rescale, luma)
    assert (got_i == want_i).all() and (got_p == want_p).all(), (what, tuple(x_host.shape), dtype, layout, rescale)
    assert (got_i.sum(axis=1) == x_host.shape[2] * x_host.shape[3]).all()
    return got_i, got_p


@pytest.mark.parametrize("T", [1, 2, 3, 9])
def test_frame_counts(T):
    _check(_data((3, T, 7, 33), f"content.T{T}"), what=f"T={T}")


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (7, 1), (5, 33), (3, 255), (3, 257), (4, 64)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_small_and_odd_frames(hw):
    _check(_data((3, 3, *hw), f"content.hw{hw}"), what=str(hw))


# one below, at and one above every partition: the thread's quad, the wave, the pass, the chunk and two chunks; H = 1 keeps the vector path
# for the multiples of 4, (n // 3) x 3 shapes would not hit n exactly
_EDGES = sorted({n + d for n in (PER_THREAD, PER_WAVE, PER_PASS, CHUNK, 2 * CHUNK) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", _EDGES)
def test_pixel_counts_at_every_partition_edge(n):
    _check(_data((3, 2, 1, n), f"content.n{n}"), what=f"1x{n}")
    if n % 4 == 0:                                          # the same count as 4 rows: row breaks inside a chunk, vector loads
        _check(_data((3, 2, 4, n // 4), f"content.n4{n}"), what=f"4x{n // 4}")
    if n % 3 == 0:
        _check(_data((3, 2, n // 3, 3), f"content.n3{n}"), what=f"{n // 3}x3")       # W = 3: a quad spans two rows


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rescale", [True, False], ids=["rescale", "unit"])
def test_dtypes_rescale_and_a_custom_luma(dtype, rescale):
    x = _data((3, 3, 9, 36), f"content.dt{dtype}{rescale}", dtype, rescale)
    _check(x, dtype, "contiguous", rescale)
    _check(x, dtype, "rows", rescale, luma=(4899, 9617, 1868, 1 << 13, 14), what="14-bit luma")
    _check(x, dtype, "contiguous", rescale, luma=(0, 1, 0, 0, 0), what="green alone")


@pytest.mark.parametrize("layout", ["rows", "offset1", "permuted", "frames"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_strided_views(layout, dtype):
    _check(_data((3, 4, 6, 40), f"content.{layout}", dtype), dtype, layout, what=layout)
    _check(_data((3, 2, 3, 33), f"content.odd.{layout}", dtype), dtype, layout, what=layout + " odd width")


def test_reversed_frames_are_refused_as_a_view_and_accepted_after_contiguous():
    x = _data((3, 4, 6, 8), "content.rev").to(DEV, torch.float16)
    with pytest.raises(_lib.HVKernelError, match="bad argument"):      # what a reversed view would hand over: a negative frame stride
        _launch(x, strides=(x.stride(0), -x.stride(1), x.stride(2)))
    rev = x.flip(1).contiguous()                            # reversed storage, non-negative strides again
    want_i, want_p = ref.histograms(x.float().cpu().numpy()[:, ::-1])
    got_i, got_p = _launch(rev)
    assert (got_i == want_i).all() and (got_p == want_p).all()
    assert (got_i == _launch(x)[0][::-1]).all() and (got_p == _launch(x)[1][::-1, ::-1]).all()   # the differences change sign


def test_refusals_leave_outputs_and_workspace_alone():
    x = torch.zeros(3, 4, 8, 16, dtype=torch.float16, device=DEV)
    need = _lib.host("content_histograms_workspace_bytes", 4, 8, 16)
    assert need == (4 * 256 + 3 * 511) * 4
    cases = {"T = 0": dict(T=0, ws_bytes=1 << 16), "row stride below W": dict(strides=(x.stride(0), x.stride(1), 15)),
             "negative channel stride": dict(strides=(-1, x.stride(1), 16)), "short workspace": dict(ws_bytes=need - 4),
             "luma above a byte": dict(luma=(9798, 19235, 3835, 1 << 14, 15)), "negative luma weight": dict(luma=(-1, 19235, 3735, 1 << 14, 15)),
             "inter NULL with T > 1": dict(inter_none=True)}
    for what, kw in cases.items():
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            _launch(x, **kw)
    q = lambda *a: _lib.host("content_histograms_workspace_bytes", *a)     # noqa: E731
    assert q(0, 8, 16) == 0 and q(65536, 8, 16) == 0 and q(4, 0, 16) == 0 and q(4, 65537, 1) == 0 and q(2, 65536, 32768) == 0
    assert q(1, 1, CHUNK) == 256 * 4 and q(1, 1, CHUNK + 1) == 2 * 256 * 4
    for bad in (torch.zeros(4, 4, 8, 16, dtype=torch.float16, device=DEV), torch.zeros(3, 4, 8, 16, dtype=torch.bfloat16, device=DEV),
                x.transpose(2, 3), x.cpu()):
        with pytest.raises(_lib.HVKernelError):
            metrics.content_histograms(bad)


def test_constant_clip_puts_every_count_in_one_bin():
    for dtype, H, W in ((torch.float16, 37, 64), (torch.float32, 9, 257)):
        gi, gp = _check(_bytes_clip(np.full((3, H, W), 200), dtype), dtype, what="constant")
        assert (gi[:, 200] == H * W).all() and gi.sum() == 3 * H * W and (gp[:, 255] == H * W).all() and gp.sum() == 2 * H * W


def test_inverting_checkerboard_fills_bins_0_and_510():
    yy, xx = np.mgrid[0:18, 0:20]
    board = ((yy + xx) & 1) * 255
    gi, gp = _check(_bytes_clip(np.stack([board, 255 - board, board])), what="checkerboard")
    assert (gp[:, 0] == 180).all() and (gp[:, 510] == 180).all() and gp.sum() == 720 and (gi[:, 0] == 180).all() and (gi[:, 255] == 180).all()


def test_random_bytes_and_a_slow_drift():
    rng = np.random.default_rng(3)
    _check(_bytes_clip(rng.integers(0, 256, size=(3, 40, 52))), what="random bytes")
    base = rng.integers(60, 180, size=(1, 40, 52))
    _check(_bytes_clip(base + rng.integers(-1, 2, size=(4, 40, 52)).cumsum(axis=0)), what="drift of +-1 per frame")


def test_4m_pixels_in_one_bin():
    x = torch.full((3, 2, 2048, 2048), 0.25, dtype=torch.float16, device=DEV)
    g = int(ref.quantised_gray(np.float32(x[0, 0, 0, 0].item())))
    intra, inter = metrics.content_histograms(x)
    assert intra.dtype == torch.int32 and inter.dtype == torch.int32 and intra.shape == (2, 256) and inter.shape == (1, 511)
    assert intra[:, g].tolist() == [1 << 22, 1 << 22] and int(intra.sum()) == 1 << 23
    assert int(inter[0, 255]) == 1 << 22 and int(inter.sum()) == 1 << 22


def test_rows_do_not_depend_on_the_other_frames_and_two_calls_agree():
    x = _data((3, 9, 24, 40), "content.slice").to(DEV, torch.float16)
    full_i, full_p = metrics.content_histograms(x)
    again_i, again_p = metrics.content_histograms(x)
    assert torch.equal(full_i, again_i) and torch.equal(full_p, again_p)
    for a, b in ((0, 0), (2, 5), (4, 8), (8, 8), (0, 8)):
        si, sp = metrics.content_histograms(x[:, a:b + 1])
        assert torch.equal(si, full_i[a:b + 1]) and torch.equal(sp, full_p[a:b]), (a, b)
    xb = torch.stack([x, x.flip(1)])                        # a batch: one launch per clip
    bi, bp = metrics.content_histograms(xb)
    assert torch.equal(bi[0], full_i) and torch.equal(bi[1], full_i.flip(0)) and torch.equal(bp[1], full_p.flip(0).flip(1))


def test_through_the_c_abi():
    lib = _lib.load()
    x = _data((3, 3, 5, 36), "content.capi").to(DEV, torch.float16)
    need = lib.hv_content_histograms_workspace_bytes(3, 5, 36)
    assert need == _lib.host("content_histograms_workspace_bytes", 3, 5, 36)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    intra = torch.full((3, 256), -1, dtype=torch.int32, device=DEV)
    inter = torch.full((2, 511), -1, dtype=torch.int32, device=DEV)
    kw = dict(x=x, sc=x.stride(0), st=x.stride(1), sh=x.stride(2), dtype=0, T=3, H=5, W=36, rescale=1, intra=intra, inter=inter, workspace=ws,
              workspace_bytes=need, **dict(zip(("wr", "wg", "wb", "round", "shift"), metrics.GRAY_LUMA)))
    args = [None if t == "hipStream_t" else (kw[p].data_ptr() if isinstance(kw[p], torch.Tensor) else kw[p]) for t, p in PARAMS["hv_content_histograms"]]
    torch.cuda.synchronize()
    assert lib.hv_content_histograms(*args) == 0
    torch.cuda.synchronize()
    want_i, want_p = ref.histograms(x.float().cpu().numpy())
    assert (intra.cpu().numpy() == want_i).all() and (inter.cpu().numpy() == want_p).all()
    out = torch.full((2, 3), SENT64, dtype=torch.float64, device=DEV)
    assert lib.hv_histogram_entropy(inter.data_ptr(), 2, 511, 255, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _compare_stats(out.cpu().numpy(), ref.row_stats(want_p, 255), "C ABI")
    assert lib.hv_histogram_entropy(inter.data_ptr(), 0, 511, 255, out.data_ptr(), None) == 0          # rows == 0: nothing done


def _compare_stats(got, want, what):
    assert got.shape == want.shape, what
    assert (got[:, 1:] == want[:, 1:]).all(), (what, "the moments are exact")
    err = float(np.abs(got[:, 0] - want[:, 0]).max()) if got.size else 0.0
    print(f"{what}: entropy error {err:.3e} bit (bound {ref.ENTROPY_TOL:.0e})")
    assert err <= ref.ENTROPY_TOL and (got[:, 0] >= 0).all(), (what, err)


def _entropy(counts, origin):
    """the finaliser between sentinels -> float64 [rows, 3]"""
    c = torch.as_tensor(np.asarray(counts), dtype=torch.int64).to(torch.int32).to(DEV).contiguous()
    rows = c.shape[0]
    buf = torch.full((rows * 3 + 16,), SENT64, dtype=torch.float64, device=DEV)
    _lib.call("histogram_entropy", poisoned_vec(c.reshape(-1)).view(c.shape), rows, c.shape[1], origin, buf[8:8 + rows * 3])
    torch.cuda.synchronize()
    assert bool((buf[:8] == SENT64).all()) and bool((buf[8 + rows * 3:] == SENT64).all())
    return buf[8:8 + rows * 3].cpu().numpy().reshape(rows, 3)


def test_entropy_finaliser_on_clip_histograms_and_hand_made_rows():
    rng = np.random.default_rng(9)
    clips = {"noise": _data((3, 5, 33, 47), "content.ent"), "bytes": _bytes_clip(rng.integers(0, 256, size=(3, 64, 64))),
             "constant": _bytes_clip(np.full((3, 8, 8), 9)),
             "drift": _bytes_clip(rng.integers(60, 180, size=(1, 40, 52)) + rng.integers(-1, 2, size=(4, 40, 52)).cumsum(axis=0))}
    for name, x in clips.items():
        wi, wp = ref.histograms(x.to(torch.float16).float().numpy())
        _compare_stats(_entropy(wi, 0), ref.row_stats(wi, 0), name + " intra")
        _compare_stats(_entropy(wp, 255), ref.row_stats(wp, 255), name + " inter")
    hand = np.zeros((6, 511), dtype=np.int64)
    hand[1, 17] = 1000                                      # a single bin
    hand[2, :] = 3                                          # all 511 bins equal
    hand[3, 0], hand[3, 510] = 5, 5
    hand[4, 255] = (1 << 31) - 1                            # the largest count of a frame
    hand[5, 0], hand[5, 510] = 1 << 30, (1 << 30) - 1       # the largest moments: N 255^2 < 2^47
    got = _entropy(hand, 255)
    _compare_stats(got, ref.row_stats(hand, 255), "hand-made rows")
    assert got[0].tolist() == [0.0, 0.0, 0.0] and got[1, 0] == 0.0 and got[3, 0] == 1.0 and got[4].tolist() == [0.0, 0.0, 0.0]
    wide = rng.integers(0, 1 << 20, size=(3, 1024))         # the widest row the finaliser takes, and a one-bin table
    _compare_stats(_entropy(wide, 0), ref.row_stats(wide, 0), "1024 bins")
    _compare_stats(_entropy(wide[:, :1], 0), ref.row_stats(wide[:, :1], 0), "1 bin")
    for bins, origin in ((1025, 0), (511, -1), (511, 512)):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            _lib.call("histogram_entropy", torch.zeros(1, bins, dtype=torch.int32, device=DEV), 1, bins, origin,
                      torch.zeros(3, dtype=torch.float64, device=DEV))


def _same_content(got, want, what):
    assert set(got) == set(want), what
    for k, v in want.items():
        if isinstance(v, float):
            assert abs(got[k] - v) <= ref.ENTROPY_TOL, (what, k, got[k], v)
        elif isinstance(v, list):
            assert len(got[k]) == len(v) and np.allclose(got[k], v, rtol=0, atol=ref.ENTROPY_TOL), (what, k)
        else:
            assert got[k] == v, (what, k, got[k], v)


def test_content_entropy_equals_the_reference_field_by_field():
    rng = np.random.default_rng(21)
    clips = [_data((3, 6, 30, 44), "content.ce"), _bytes_clip(rng.integers(90, 110, size=(5, 33, 31))), _data((3, 1, 9, 12), "content.single"),
             _bytes_clip(np.full((2, 8, 8), 77))]
    devs = [x.to(DEV, torch.float16) for x in clips]
    wants = [ref.content_entropy(d.float().cpu().numpy()) for d in devs]
    for d, w in zip(devs, wants):
        _same_content(metrics.content_entropy(d), w, tuple(d.shape))
    assert wants[2]["inter_entropy"] is None and metrics.content_bucket(metrics.content_entropy(devs[2])["inter_entropy"]) is None
    many = metrics.content_entropy_many(iter(devs))         # everything enqueued, one synchronisation
    for m, w in zip(many, wants):
        _same_content(m, w, "many")
    _same_content(metrics.content_entropy(devs[0][None]), wants[0], "[1,3,T,H,W]")
    with pytest.raises(_lib.HVKernelError, match="one clip"):
        metrics.content_entropy(torch.stack([devs[0], devs[0]]))


def _load_script(rel):
    spec = importlib.util.spec_from_file_location("hv_content_gpu_" + os.path.basename(rel)[:-3], os.path.join(ROOT, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_driver_flags_end_to_end(tmp_path, capsys):
    rng = np.random.default_rng(2)
    src = tmp_path / "in"
    src.mkdir()
    still = np.broadcast_to(rng.integers(0, 256, size=(1, 32, 32)), (5, 32, 32))
    clips = {"calm": _bytes_clip(np.array(still)), "busy": _bytes_clip(rng.integers(0, 256, size=(5, 32, 32)))}
    for name, x in clips.items():
        torch.save(x.to(torch.float16), src / f"{name}.pt")

    # tools/bucket_clips.py on the device: the records equal the reference, the lists carry the fork's names
    tool = _load_script("tools/bucket_clips.py")
    bdir = tmp_path / "buckets"
    recs = tool.main(["--tensor-dir", str(src), "--output-dir", str(bdir)])
    assert [r["name"] for r in recs] == ["busy", "calm"]
    for r in recs:
        _same_content({k: r[k] for k in ref.content_of_gray(np.zeros((1, 1)))}, ref.content_entropy(clips[r["name"]].half().float().numpy()), r["name"])
    assert {r["name"]: r["bucket"] for r in recs} == {"busy": "High_InterEntropy_gt6", "calm": "Very_Low_InterEntropy_lt2"}
    assert sorted(f for f in os.listdir(bdir)) == ["High_InterEntropy_gt6.txt", "Very_Low_InterEntropy_lt2.txt", "content.jsonl"]
    assert open(bdir / "High_InterEntropy_gt6.txt").read() == str(src / "busy.pt") + "\n"

    # infer.py --score --content
    infer = _load_script("infer.py")
    base = ["--tensor-dir", str(src), "--reduced", "--config-json", T_OPS, "--score"]
    infer.main(base + ["--output-dir", str(tmp_path / "plain")])
    infer.main(base + ["--output-dir", str(tmp_path / "out"), "--content"])
    names = lambda d: [f for f in _tree(d) if not f.startswith("metrics_")]      # noqa: E731  (the result file carries a timestamp)
    assert names(tmp_path / "plain") == ["busy.pt", "calm.pt"]                   # without the flag: today's files, nothing else
    assert names(tmp_path / "out") == ["busy.pt", "busy_content.json", "calm.pt", "calm_content.json"]
    for f in ("busy.pt", "calm.pt"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "out" / f, "rb").read()
    for name in clips:
        js = json.load(open(tmp_path / "out" / f"{name}_content.json"))
        assert set(js) == {"input", "reconstruction"} and js["input"]["definition"] == ref.DEFINITION
        _same_content(js["input"], ref.content_entropy(clips[name].half().float().numpy()), name)
        assert js["reconstruction"]["frames"] >= 1 and js["reconstruction"]["intra_entropy"] >= 0.0
    assert "Content busy: inter-frame entropy input" in capsys.readouterr().out

    # tools/run_vae_study.py: --content adds one key, --bucket-dir one tree per list; without them nothing changes
    study = _load_script("tools/run_vae_study.py")
    common = ["--tensor-dir", str(src), "--base-config", T_OPS, "--mode", "pool", "--limit", "2", "--reduced"]
    plain = study.main(common + ["--output-dir", str(tmp_path / "s0")])
    cont = study.main(common + ["--output-dir", str(tmp_path / "s1"), "--content"])
    assert [f for f in _tree(tmp_path / "s0") if not f.startswith("config_")] == ["study.jsonl"]
    assert _tree(tmp_path / "s0") == _tree(tmp_path / "s1")                      # --content adds a key to the records, no file
    seen = 0
    for p, c in zip(plain, cont):
        if "refused" in p:
            assert c == p
            continue
        seen += 1
        assert set(p) == {"config", "PSNR", "SSIM", "frames", "compression"}               # today's keys, nothing else
        assert set(c) == set(p) | {"content"} and all(c[k] == p[k] for k in p)
        k = c["content"]
        assert set(k) == {"input", "reconstruction", "clips", "definition", "inter_entropy_drop"} and k["clips"] == 2
        want = [ref.content_entropy(clips[n].half().float().numpy()) for n in ("busy", "calm")]
        for f in ("inter_entropy", "intra_entropy", "mean_abs_diff", "ti"):
            assert abs(k["input"][f] - (want[0][f] + want[1][f]) / 2) <= ref.ENTROPY_TOL, f
        assert k["inter_entropy_drop"] == k["input"]["inter_entropy"] - k["reconstruction"]["inter_entropy"]
    assert seen >= 1
    bucketed = study.main(common + ["--output-dir", str(tmp_path / "s2"), "--bucket-dir", str(bdir), "--content"])
    assert len(bucketed) == 4 and [r["bucket"] for r in bucketed] == ["High_InterEntropy_gt6"] * 2 + ["Very_Low_InterEntropy_lt2"] * 2
    for b, name in (("High_InterEntropy_gt6", "busy"), ("Very_Low_InterEntropy_lt2", "calm")):
        lines = [json.loads(ln) for ln in open(tmp_path / "s2" / b / "study.jsonl")]
        assert lines == [r for r in bucketed if r["bucket"] == b]
        for r in lines:
            if "refused" not in r:
                assert r["content"]["clips"] == 1
                assert abs(r["content"]["input"]["inter_entropy"] - ref.content_entropy(clips[name].half().float().numpy())["inter_entropy"]) <= ref.ENTROPY_TOL
    assert not os.path.exists(tmp_path / "s2" / "study.jsonl")
    (bdir / "Low_InterEntropy_2-4.txt").write_text("missing_clip.mp4\n")
    with pytest.raises(ValueError, match="missing_clip"):
        study.main(common + ["--output-dir", str(tmp_path / "s3"), "--bucket-dir", str(bdir)])
