"""Block-matching motion fields on the GPU (csrc/hv_motion.hip) against the numpy restatement tests/motion_ref.py: mv, sad and sad0 bit
for bit through torch.ops.hv.block_motion and the C ABI, at partial blocks, single blocks, W = 1, exact tilings, windows wider than the
frame, every radius parity, T = 1 / 2 / 5, both dtypes, strided views, both quantisers, another luma, lam 0 / default / 255, on noise,
constant, striped, shifted, saturated and slowly drifting content; guarded outputs, two runs, slice invariance, and metrics.motion_compare
end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _abi, _lib, metrics  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from tests import motion_ref as ref  # noqa: E402
from tests.guarded_memory import INT, NAN_BITS, GuardedFlat, poisoned_vec  # noqa: E402

DEV = "cuda:0"
_DT = {torch.float16: 0, torch.float32: 1}
PARAMS = {name: params for _, name, params in _abi.MOTION_DECLS}
_REF = {}                                   # reference fields, computed once per (content, geometry) and never changed


def _noise(shape, key, dtype=torch.float16, rescale=True):
    """host float32 values that `dtype` holds exactly, a little beyond the quantiser's range on both sides"""
    x = syn.hashed_uniform(shape, key, 0)
    x = 1.1 * x / x.abs().max()
    if not rescale:
        x = x.abs() * 1.05 - 0.02
    return x.to(dtype).float()


def _bytes_clip(q):
    """bytes [T, H, W] -> float32 [3, T, H, W] in [-1, 1], exact in fp16, whose gray frames (rescale, default luma) are q"""
    x = ((torch.as_tensor(np.array(q), dtype=torch.float64) + 0.5) / 255.0 * 2.0 - 1.0).to(torch.float16)
    return x[None].expand(3, *x.shape).contiguous().float()


def _rand_bytes(shape, key):
    u = syn.hashed_uniform(shape, key, 0).numpy().astype(np.float64)
    u = (u - u.min()) / (u.max() - u.min())
    return np.minimum((u * 256).astype(np.int64), 255)


def _content(kind, T, H, W):
    """float32 [3, T, H, W] of one of the issue's contents"""
    if kind == "noise":
        return _noise((3, T, H, W), f"motion.noise.{T}.{H}.{W}")
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "constant":
        q = np.full((T, H, W), 77)
    elif kind == "stripes":
        q = np.broadcast_to((xx % 4) * 60, (T, H, W))
    elif kind == "shifted":                 # frame t + 1 is frame t moved by (2, -3), replicated edges
        frames = [_rand_bytes((H, W), f"motion.tex.{H}.{W}")]
        for _ in range(T - 1):
            frames.append(ref.shifted(frames[-1], 2, -3))
        q = np.stack(frames)
    elif kind == "saturation":              # 0 against 255, alternating
        q = np.stack([np.full((H, W), 255 * (t % 2)) for t in range(T)])
    elif kind == "ramp":                    # a slow diagonal ramp drifting by one pixel a frame: many near-ties
        q = np.stack([((xx + 2 * yy + t) // 3) % 256 for t in range(T)])
    else:
        raise ValueError(kind)
    return _bytes_clip(q)


def _layout(x, kind):
    """x [3,T,H,W] on the device -> a view with the same values inside NaN-filled memory"""
    C, T, H, W = x.shape
    nan, it = NAN_BITS[x.element_size()], INT[x.element_size()]
    if kind == "contiguous":
        return poisoned_vec(x.contiguous().reshape(-1)).view(C, T, H, W)
    if kind == "rows":                       # row stride above W, every other row of a taller buffer
        buf = torch.full((C, T, 2 * H + 1, W + 8), nan, dtype=it, device=x.device).view(x.dtype)
        v = buf[:, :, 1:2 * H:2, 4:4 + W]
    elif kind == "offset1":                  # the view starts one element into a row
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


def _launch(x, block, radius, lam, rescale=True, luma=metrics.GRAY_LUMA, null=False):
    """one call through torch.ops.hv with guarded outputs -> (mv int16 [P,Hb,Wb,2], sad, sad0 int64 [P,Hb,Wb]) numpy"""
    _, T, H, W = x.shape
    Hb, Wb = ref.blocks(H, W, block)
    n = (T - 1) * Hb * Wb
    mv, sad, sad0 = GuardedFlat(max(2 * n, 2), torch.int16), GuardedFlat(max(n, 1), torch.int32), GuardedFlat(max(n, 1), torch.int32)
    before = [g.buf.clone() for g in (mv, sad, sad0)]
    _lib.call("block_motion", x, x.stride(0), x.stride(1), x.stride(2), _DT[x.dtype], T, H, W, 1 if rescale else 0, *luma, block, radius, lam,
              None if null else mv.view, None if null else sad.view, None if null else sad0.view)
    torch.cuda.synchronize()
    assert mv.intact() and sad.intact() and sad0.intact(), "a write outside the outputs"
    if T == 1:
        assert all(torch.equal(g.buf, b) for g, b in zip((mv, sad, sad0), before)), "T = 1 wrote to an output"
    return (mv.view.cpu().numpy()[:2 * n].reshape(T - 1, Hb, Wb, 2), sad.view.cpu().numpy()[:n].astype(np.int64).reshape(T - 1, Hb, Wb),
            sad0.view.cpu().numpy()[:n].astype(np.int64).reshape(T - 1, Hb, Wb))


def _want(key, x_host, block, radius, lam, rescale=True, luma=metrics.GRAY_LUMA):
    k = (key, block, radius, lam, rescale, tuple(luma))
    if k not in _REF:
        _REF[k] = ref.block_motion(x_host.numpy(), block, radius, lam, rescale, luma)
        for a in _REF[k]:
            a.setflags(write=False)
    return _REF[k]


def _same(got, want, what):
    for name, g, w in zip(("mv", "sad", "sad0"), got, want):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w.astype(g.dtype))
        assert bad.size == 0, (what, name, f"{len(bad)} cells differ, first {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}")


def _check(key, x_host, block, radius, lam=None, dtype=torch.float16, layout="contiguous", rescale=True, luma=metrics.GRAY_LUMA):
    lam = ref.default_lam(block) if lam is None else lam
    x_host = x_host.to(dtype).float()                    # the values the device holds
    want = _want((key, dtype), x_host, block, radius, lam, rescale, luma)
    got = _launch(_layout(x_host.to(DEV, dtype), layout), block, radius, lam, rescale, luma)
    _same(got, want, (key, block, radius, lam, dtype, layout, rescale))
    return got


# H, W, block, radius: partial blocks of 1 row / 15 columns (33 x 47) and 5 rows / 2 columns (37 x 50); a single partial block and W = 1;
# exact tilings of the 32 x 32 workgroup tile and of the blocks; a window wider than the frame (every side clamped); radius 1; odd radii
# (the window's row length rounds differently); the largest radius with both blocks
_SHAPES = [(33, 47, 16, 8), (37, 50, 16, 8), (37, 50, 8, 7), (7, 5, 8, 4), (7, 5, 16, 4), (16, 1, 8, 4), (16, 1, 16, 4), (48, 64, 16, 8),
           (48, 64, 8, 5), (40, 40, 16, 32), (40, 40, 8, 32), (33, 47, 16, 1), (33, 47, 8, 1), (35, 70, 16, 31), (33, 33, 16, 16)]


@pytest.mark.parametrize("H,W,block,radius", _SHAPES, ids=lambda v: str(v))
def test_shapes_on_noise(H, W, block, radius):
    _check(f"noise.{H}.{W}", _content("noise", 2, H, W), block, radius)


@pytest.mark.parametrize("kind", ["noise", "constant", "stripes", "shifted", "saturation", "ramp"])
@pytest.mark.parametrize("block", [8, 16])
def test_contents(kind, block):
    H, W, R = 37, 50, 8
    mv, sad, sad0 = _check(f"{kind}.3.{H}.{W}", _content(kind, 3, H, W), block, R)
    if kind in ("constant", "stripes"):
        assert not mv.any() and not sad.any() and not sad0.any()
    if kind == "saturation":
        assert not mv.any() and (sad == sad0).all() and sad[0, 0, 0] == block * block * 255
    if kind == "shifted":
        assert not sad.any()
        Hb, Wb = ref.blocks(H, W, block)
        # blocks whose pixels and matched pixels lie inside the frame: rows by*B + 2 + B - 1 <= H - 1, columns bx*B - 3 >= 0
        inner = mv[:, :(H - 2) // block, 1:(W // block)]
        assert (inner[..., 0] == 2).all() and (inner[..., 1] == -3).all()


@pytest.mark.parametrize("lam", [0, None, 255], ids=["lam0", "default", "lam255"])
@pytest.mark.parametrize("kind", ["noise", "ramp", "shifted"])
def test_lam(kind, lam):
    _check(f"{kind}.3.37.50", _content(kind, 3, 37, 50), 16, 8, lam)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("rescale", [True, False], ids=["rescale", "unit"])
def test_dtypes_rescale_and_a_custom_luma(dtype, rescale):
    x = _noise((3, 3, 19, 36), f"motion.dt{dtype}{rescale}", dtype, rescale)
    key = f"dt.{rescale}"
    _check(key, x, 16, 6, dtype=dtype, rescale=rescale)
    _check(key, x, 8, 6, dtype=dtype, layout="rows", rescale=rescale, luma=(4899, 9617, 1868, 1 << 13, 14))
    _check(key, x, 8, 3, dtype=dtype, rescale=rescale, luma=(0, 1, 0, 0, 0))


@pytest.mark.parametrize("layout", ["rows", "offset1", "permuted", "frames"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_strided_views(layout, dtype):
    _check("views", _noise((3, 3, 21, 40), "motion.views"), 16, 5, dtype=dtype, layout=layout)
    _check("views.odd", _noise((3, 2, 9, 33), "motion.views.odd"), 8, 4, dtype=dtype, layout=layout)


def test_a_single_frame_writes_nothing_and_takes_null_outputs():
    x = _noise((3, 1, 9, 20), "motion.T1").to(DEV, torch.float16)
    for null in (False, True):
        mv, sad, sad0 = _launch(x, 16, 8, 16, null=null)
        assert mv.shape == (0, 1, 2, 2) and sad.shape == (0, 1, 2)
    mv, sad, sad0 = metrics.block_motion(x)
    assert mv.shape == (0, 1, 2, 2) and sad.shape == sad0.shape == (0, 1, 2)
    assert metrics.motion_stats(x)["motion_mean"] is None


def test_a_pair_depends_on_its_two_frames_only():
    x = _content("ramp", 5, 33, 47) + 0.25 * _noise((3, 5, 33, 47), "motion.T5")
    whole = _check("T5", x, 16, 6)
    xd = x.to(DEV, torch.float16)
    for t in range(4):
        part = _launch(xd[:, t:t + 2], 16, 6, 16)
        for w, p in zip(whole, part):
            assert (w[t] == p[0]).all(), t


def test_two_runs_give_the_same_bits():
    x = _content("ramp", 3, 37, 50).to(DEV, torch.float16)
    a, b = _launch(x, 16, 16, 16), _launch(x, 16, 16, 16)
    assert all((p == q).all() for p, q in zip(a, b))


def test_null_outputs_and_bad_parameters_are_refused_and_write_nothing():
    x = torch.zeros(3, 2, 8, 16, dtype=torch.float16, device=DEV)
    for kw in (dict(null=True), dict(block=12), dict(radius=0), dict(radius=33), dict(lam=-1), dict(lam=256)):
        args = dict(block=16, radius=8, lam=16)
        args.update(kw)
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            _launch(x, args["block"], args["radius"], args["lam"], null=args.get("null", False))
    out = torch.full((2 * 1 * 1 * 2 + 1,), 0x7E5A, dtype=torch.int16, device=DEV)
    sad = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HVKernelError, match="bad argument"):      # mv two bytes off its alignment
        _lib.call("block_motion", x, x.stride(0), x.stride(1), x.stride(2), 0, 2, 8, 16, 1, *metrics.GRAY_LUMA, 16, 8, 16, out[1:], sad, sad)
    torch.cuda.synchronize()
    assert (out == 0x7E5A).all() and not sad.any()


def test_through_the_c_abi():
    lib = _lib.load()
    x_host = _noise((3, 3, 21, 36), "motion.capi")
    x = x_host.to(DEV, torch.float16)
    Hb, Wb = ref.blocks(21, 36, 8)
    mv = torch.full((2, Hb, Wb, 2), -999, dtype=torch.int16, device=DEV)
    sad = torch.full((2, Hb, Wb), -1, dtype=torch.int32, device=DEV)
    sad0 = torch.full((2, Hb, Wb), -1, dtype=torch.int32, device=DEV)
    kw = dict(x=x, sc=x.stride(0), st=x.stride(1), sh=x.stride(2), dtype=0, T=3, H=21, W=36, rescale=1, block=8, radius=5, lam=3, mv=mv,
              sad=sad, sad0=sad0, **dict(zip(("wr", "wg", "wb", "round", "shift"), metrics.GRAY_LUMA)))
    args = [None if t == "hipStream_t" else (kw[p].data_ptr() if isinstance(kw[p], torch.Tensor) else kw[p]) for t, p in PARAMS["hv_block_motion"]]
    torch.cuda.synchronize()
    assert lib.hv_block_motion(*args) == 0
    torch.cuda.synchronize()
    want = _want(("capi", torch.float16), x.float().cpu(), 8, 5, 3)
    _same((mv.cpu().numpy(), sad.cpu().numpy().astype(np.int64), sad0.cpu().numpy().astype(np.int64)), want, "C ABI")
    kw.update(T=1, mv=None, sad=None, sad0=None)                       # T == 1: NULL outputs, HV_OK
    args = [None if t == "hipStream_t" else (kw[p].data_ptr() if isinstance(kw[p], torch.Tensor) else kw[p]) for t, p in PARAMS["hv_block_motion"]]
    assert lib.hv_block_motion(*args) == 0


def test_metrics_end_to_end():
    x_host = _content("shifted", 4, 37, 50)
    x = x_host.to(DEV, torch.float16)
    mv, sad, sad0 = (t.cpu().numpy() for t in metrics.block_motion(x[None], block=16, radius=8))
    want = _want(("shifted.e2e", torch.float16), x.float().cpu(), 16, 8, 16)
    _same((mv, sad.astype(np.int64), sad0.astype(np.int64)), want, "metrics.block_motion")
    stats = metrics.motion_stats(x, block=16, radius=8)
    assert stats == metrics.motion_from_host(*want, 8, 16, 16)
    assert stats["definition"] == metrics.MOTION_DEFINITION and "not FVMD" in stats["definition"]
    assert stats["frames"] == 4 and stats["motion_max"] >= np.sqrt(13.0) and 0.0 < stats["mc_gain"] <= 1.0
    many = metrics.motion_stats_many([x, x[:, :1], x[:, 1:3]], block=16, radius=8)
    assert many[0] == stats and many[1]["motion_mean"] is None and many[2]["frames"] == 2
    same = metrics.motion_compare(x, x, block=16, radius=8)
    assert same["motion_epe"] == 0.0 and same["motion_mean_change"] == 0.0 and same["ref"] == same["rec"] == stats
    still = x[:, :1].expand(3, 3, 37, 50)                               # a frozen reconstruction, one frame shorter: a view with st = 0
    cmp = metrics.motion_compare(x, still, block=16, radius=8)
    assert cmp["rec"]["motion_mean"] == 0.0 and cmp["rec"]["static_share"] == 1.0 and cmp["ref"]["frames"] == cmp["rec"]["frames"] == 3
    assert cmp["motion_epe"] == pytest.approx(cmp["ref"]["motion_mean"]) and cmp["motion_mean_change"] == -cmp["ref"]["motion_mean"]
    summary = metrics.motion_summary([stats], [cmp])
    assert summary["motion_epe"] == cmp["motion_epe"] and summary["clips"] == 1 and summary["definition"] == metrics.MOTION_DEFINITION
    with pytest.raises(_lib.HVKernelError, match="differ in more than the frame count"):
        metrics.motion_compare(x, x[:, :, :-1])
    with pytest.raises(_lib.HVKernelError, match="GPU tensor"):
        metrics.block_motion(x.cpu())


def _load_script(rel):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("hv_motion_gpu_" + os.path.basename(rel)[:-3], os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_flags_end_to_end(tmp_path, capsys):
    import json
    import os
    t_ops = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t_ops_config.json")
    src = tmp_path / "in"
    src.mkdir()
    P = _rand_bytes((32, 32), "motion.drivers")
    frames = [P]
    for _ in range(4):
        frames.append(ref.shifted(frames[-1], 0, 2))
    clips = {"pan": _bytes_clip(np.stack(frames)), "still": _bytes_clip(np.stack([P] * 5))}
    for name, x in clips.items():
        torch.save(x.to(torch.float16), src / f"{name}.pt")
    want = {n: metrics.motion_from_host(*ref.block_motion(x.half().float().numpy(), 8, 4, 4), 4, 8, 4) for n, x in clips.items()}
    flags = ["--motion", "--motion-block", "8", "--motion-radius", "4"]
    tree = lambda d: sorted(f for f in os.listdir(d) if not f.startswith(("metrics_", "config_")))      # noqa: E731

    # tools/bucket_clips.py --metric motion on the device: the records equal the reference
    tool = _load_script("tools/bucket_clips.py")
    recs = tool.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / "b"), "--metric", "motion", "--edges", "1", "--motion-block", "8",
                      "--motion-radius", "4"])
    assert {r["name"]: r["bucket"] for r in recs} == {"pan": "B1_Motion_gt1", "still": "B0_Motion_lt1"}
    for r in recs:
        assert all(r[k] == v for k, v in want[r["name"]].items()), r["name"]

    # infer.py --score --motion: one more file per clip, the others unchanged
    infer = _load_script("infer.py")
    base = ["--tensor-dir", str(src), "--reduced", "--config-json", t_ops, "--score"]
    infer.main(base + ["--output-dir", str(tmp_path / "plain")])
    infer.main(base + ["--output-dir", str(tmp_path / "out")] + flags)
    assert tree(tmp_path / "plain") == ["pan.pt", "still.pt"]
    assert tree(tmp_path / "out") == ["pan.pt", "pan_motion.json", "still.pt", "still_motion.json"]
    for f in ("pan.pt", "still.pt"):
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "out" / f, "rb").read()
    for name in clips:
        js = json.load(open(tmp_path / "out" / f"{name}_motion.json"))
        n = js["ref"]["frames"]                               # the frames both have: a configuration may shorten the clip
        assert js["definition"] == metrics.MOTION_DEFINITION and js["rec"]["frames"] == n and 2 <= n <= 5
        assert js["ref"]["motion_pairs"] == want[name]["motion_pairs"][:n - 1] and (n < 5 or js["ref"] == want[name])
        assert js["motion_epe"] >= 0.0 and js["motion_mean_change"] == js["rec"]["motion_mean"] - js["ref"]["motion_mean"]
    assert "Motion pan: input 1.9" in capsys.readouterr().out and 1.9 < want["pan"]["motion_mean"] < 2.0 and want["still"]["motion_mean"] == 0.0

    # tools/run_vae_study.py --motion: one more key per record
    study = _load_script("tools/run_vae_study.py")
    common = ["--tensor-dir", str(src), "--base-config", t_ops, "--mode", "pool", "--limit", "2", "--reduced"]
    plain = study.main(common + ["--output-dir", str(tmp_path / "s0")])
    moved = study.main(common + ["--output-dir", str(tmp_path / "s1")] + flags)
    assert tree(tmp_path / "s0") == tree(tmp_path / "s1") == ["study.jsonl"]
    seen = 0
    for p, c in zip(plain, moved):
        if "refused" in p:
            assert c == p
            continue
        seen += 1
        assert set(c) == set(p) | {"motion"} and all(c[k] == p[k] for k in p)
        m = c["motion"]
        assert m["clips"] == 2 and (m["block"], m["radius"], m["lam"]) == (8, 4, 4) and m["definition"] == metrics.MOTION_DEFINITION
        assert m["input"]["motion_mean"] == (want["pan"]["motion_mean"] + want["still"]["motion_mean"]) / 2
        assert m["motion_epe"] >= 0.0 and m["reconstruction"]["motion_mean"] is not None
    assert seen >= 1

    # evaluation/compute_metrics.py --motion: two more lines, only when asked
    cm = _load_script("evaluation/compute_metrics.py")
    roots = ["--root1", str(src), "--root2", str(tmp_path / "out")]
    text = open(cm.main(roots + ["--results-dir", str(tmp_path / "r0")])[0]).read()
    assert "Motion" not in text
    text = open(cm.main(roots + ["--results-dir", str(tmp_path / "r1")] + flags)[0]).read()
    assert "\nMotionEPE: " in text and "\nMotionMean: " in text and "not FVMD" in text
