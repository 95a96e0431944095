"""GPU: LPIPS (AlexNet) scoring - csrc/hv_lpips.hip through the C ABI kernel by kernel, and metrics.lpips_video end to end - against
the float64 restatement tests/lpips_ref.py.  Weights are LpipsAlex.synthetic (conv hashed_uniform * sqrt(6 / fan_in), bias
0.1 * hashed_uniform, lin 0.5 * |hashed_uniform|): about half the units are live and every tap contributes.

Bounds.
  * conv: each kernel gets the GPU's own previous-layer output (layer 1: the quantised bytes through the LUT) and is compared element
    by element with the fp64 conv of those operands under tests/error_bounds.py (Ref.add per tap, bound(torch.float32)): the MFMA is
    an fp32 fma chain, the model that statistical bound assumes; ReLU is 1-Lipschitz, so |relu(got) - relu(y64)| obeys the bound of y64.
    The k step is 32: K = 363 leaves a tail of 11 (zero-padded to 384), 1600, 1728, 3456 and 2304 are whole multiples.
  * maxpool: exact.
  * layer distance: against fp64 on the same features, within 4 * sqrt(C) * 2^-24 of sum_c lin (n0^2 + n1^2) per frame.
  * end to end: |GPU - fp64| <= max(16 * e32, 4 * sqrt(3456) * 2^-24 * |v64|), e32 = |fp32 restatement - fp64 restatement|."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _lib, metrics  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from hunyuanvideo_efficiency_amd.metrics import LPIPS_CHNS, LPIPS_CONVS, LpipsAlex  # noqa: E402
from tests import error_bounds as eb  # noqa: E402
from tests import lpips_ref, metrics_ref  # noqa: E402
from tests.guarded_memory import GuardedFlat, crop, poisoned_vec  # noqa: E402

DEV = "cuda:0"
_MODEL = None


def _model():
    global _MODEL
    if _MODEL is None:
        _MODEL = LpipsAlex.synthetic(0)
    return _MODEL


def _video(shape, key, unit=False):
    x = syn.hashed_uniform(shape, key, 0)
    x = x / x.abs().max()
    return (x.abs() if unit else x).half()


def _pair(shape, key, noise, unit=False):
    """fp16-representable (ref, rec) on the host; rec = ref + noise * another video"""
    a = _video(shape, key + ".a", unit)
    b = (a.float() + noise * _video(shape, key + ".b").float()).half()
    return a, b


def _strided(x, kind):
    """as tests/test_gpu_metrics.py: `t` - every other frame of a longer buffer; `h` - rows of a taller, wider buffer (row stride > W,
    an odd element offset)"""
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


def _poisoned_weights(model):
    """the packed device weights, each followed by NaNs"""
    w = model.on(DEV)
    return {"w": [poisoned_vec(t.reshape(-1)) for t in w["w"]], "b": [poisoned_vec(t) for t in w["b"]],
            "lin": [poisoned_vec(t) for t in w["lin"]], "lut": poisoned_vec(w["lut"].reshape(-1))}


def _conv_ref(x_cl, w, b, stride, pad):
    """x_cl [N, H, W, Cin] fp64 (host), torch weight [Cout, Cin, k, k] -> error_bounds.Ref over rows (n, oy, ox), one K-slice per tap"""
    N, H, W, Cin = x_cl.shape
    k = w.shape[-1]
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, Cin, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W] = x_cl
    ref = eb.Ref()
    for ky in range(k):
        for kx in range(k):
            a = xp[:, ky:ky + stride * (OH - 1) + 1:stride, kx:kx + stride * (OW - 1) + 1:stride].reshape(N * OH * OW, Cin)
            ref.add(a, w[:, :, ky, kx])
    return ref.bias(b), OH, OW


def _check_conv(got, ref, what):
    """got [M, Cout] after ReLU against relu(y64), within the bound of y64"""
    g = got.double().cpu()
    r = (g - ref.y.clamp(min=0.0)).abs() / ref.bound(torch.float32)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
    worst = float(r.max())
    live = float((g > 0).double().mean())
    print(f"{what}: K {ref.k} rows {g.shape[0]} worst error / bound {worst:.3f}, live units {live:.2f}")
    assert worst <= 1.0, f"{what}: {int((r > 1).sum())} of {r.numel()} elements outside the fp64 bound (worst {worst:.3g})"
    assert 0.1 < live < 0.9, (what, live)                    # the test data exercises both sides of the ReLU
    return worst


CONV_SHAPES = [(1, 31, 31), (1, 31, 35), (1, 34, 47), (1, 38, 43), (3, 90, 160)]


@pytest.mark.parametrize("T,H,W", CONV_SHAPES)
def test_each_conv_and_pool_alone_against_fp64(T, H, W):
    """the five conv launches and the two pools of one chunk, each on the GPU's own previous output, operands in NaN-poisoned buffers and
    outputs in guarded ones.  31x31: maps 7, 3, 1, 1, 1 (a single ragged M tile); 3 x 90x160: 6 images of 21x39 rows - several M tiles,
    tiles that straddle images, a ragged last one."""
    model = _model()
    wts = _poisoned_weights(model)
    a, b = _pair((3, T, H, W), f"lpips.conv.{T}x{H}x{W}", 0.1)
    vids = []
    for v in (a, b):
        _, view, _ = crop((3, T, H, W), torch.float16, None)
        view.copy_(v.to(DEV))
        vids.append(view)
    sizes = metrics.lpips_map_sizes(H, W)
    N = 2 * T
    # layer 1 operands: the LUT value of every quantised byte, images = frames of a, then frames of b
    lut = metrics.lpips_lut().double()
    q = np.concatenate([metrics_ref.quantise(v.float().numpy()) for v in (a, b)], axis=1)             # [3, 2T, H, W]
    qi = torch.from_numpy(q).long()
    x = torch.stack([lut[c][qi[c]] for c in range(3)], dim=-1)                                          # [2T, H, W, 3]
    gpu_in = None
    for layer, (_, ci, co, k, stride, pad) in enumerate(LPIPS_CONVS):
        h, w = sizes[layer]
        out = GuardedFlat(N * h * w * co, torch.float32)
        if layer == 0:
            va, vb = vids
            _lib.call("lpips_conv1_f32", va, va.stride(0), va.stride(1), va.stride(2), vb, vb.stride(0), vb.stride(1), vb.stride(2), 0,
                      T, H, W, 1, wts["lut"], wts["w"][0], wts["b"][0], out.view)
        else:
            _lib.call("lpips_conv2d_f32", gpu_in, wts["w"][layer], wts["b"][layer], out.view, N, h, w, ci, co, k, pad)
            x = gpu_in.double().cpu().reshape(N, h, w, ci)
        ref, oh, ow = _conv_ref(x, model.convs[layer][0], model.convs[layer][1], stride, pad)
        assert (oh, ow) == (h, w)
        assert out.intact(), f"layer {layer + 1}: wrote outside its output"
        _check_conv(out.view.reshape(N * h * w, co), ref, f"{T}x{H}x{W} conv{layer + 1}")
        gpu_in = out.view
        if layer < 2:                                            # maxpool 3/2, exact against torch on the same input
            ph, pw = sizes[layer + 1]
            pooled = GuardedFlat(N * ph * pw * co, torch.float32)
            _lib.call("lpips_maxpool_f32", gpu_in, pooled.view, N, h, w, co)
            want = F.max_pool2d(gpu_in.reshape(N, h, w, co).permute(0, 3, 1, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1)
            assert tuple(want.shape) == (N, ph, pw, co) and pooled.intact()
            assert torch.equal(pooled.view.reshape(N, ph, pw, co), want), f"{T}x{H}x{W} pool after tap {layer + 1}"
            gpu_in = pooled.view


@pytest.mark.parametrize("N,H,W,C", [(2, 8, 10, 64), (3, 7, 7, 192), (1, 3, 3, 4), (2, 21, 39, 64), (1, 4, 5, 384)])
def test_maxpool_exact_where_the_floor_drops_a_row_or_column(N, H, W, C):
    """8 -> 3 and 10 -> 4 leave the last row / column unread; 4 x 5 -> 1 x 2; signed values"""
    x = poisoned_vec(syn.hashed_uniform((N * H * W * C,), f"lpips.pool.{N}.{H}.{W}.{C}", 0).to(DEV))
    oh, ow = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = GuardedFlat(N * oh * ow * C, torch.float32)
    _lib.call("lpips_maxpool_f32", x, y.view, N, H, W, C)
    want = F.max_pool2d(x.reshape(N, H, W, C).permute(0, 3, 1, 2), kernel_size=3, stride=2).permute(0, 2, 3, 1)
    assert y.intact() and torch.equal(y.view.reshape(N, oh, ow, C), want)


def _out_buffer(T):
    """fp64 [T, 5] behind and in front of sentinel words"""
    buf = torch.full((T * 5 + 16,), 0x7F5A5A5A7F5A5A5A, dtype=torch.int64, device=DEV)
    return buf, buf.view(torch.float64)[8:8 + T * 5].reshape(T, 5)


def _distance(f, lin, T, P, C, layer):
    buf, out = _out_buffer(T)
    nbytes = _lib.host("lpips_distance_workspace_bytes", T, P)
    ws = GuardedFlat(nbytes, torch.uint8, front=16)
    _lib.call("lpips_distance_f32", f, lin, T, P, C, layer, out, ws.view, nbytes)
    torch.cuda.synchronize()
    keep = torch.ones(T * 5 + 16, dtype=torch.bool, device=DEV)
    keep[8 + layer:8 + T * 5:5] = False
    assert bool((buf[keep] == 0x7F5A5A5A7F5A5A5A).all()) and ws.intact(), "wrote outside its column / workspace"
    return out[:, layer].cpu().numpy()


@pytest.mark.parametrize("P,C,layer", [(1, 384, 2), (56, 64, 0), (819, 192, 1), (17001, 64, 0), (36, 256, 4)])
def test_layer_distance_against_fp64_and_zero_pixels(P, C, layer):
    """P = 1: one pixel, one workgroup; 819: 13 workgroups; 17001: more pixels than 4 x 256 waves, a ragged last round.  A fifth of the
    pixels are all zero in both images (0 / (0 + 1e-10) = 0, not NaN), a tenth in one image only."""
    T = 3
    f = syn.hashed_uniform((2 * T, P, C), f"lpips.dist.{P}.{C}", 0).clamp(min=0.0)           # post-ReLU-like: half the units live
    sel = syn.hashed_uniform((2 * T, P), f"lpips.dist.zero.{P}.{C}", 0)
    if P > 1:
        f[sel < -0.8] = 0.0
        both = sel[:T] < -0.6
        f[:T][both] = 0.0
        f[T:][both] = 0.0
    lin = 0.5 * syn.hashed_uniform((C,), f"lpips.dist.lin.{C}", 0).abs()
    got = _distance(poisoned_vec(f.reshape(-1).to(DEV)), poisoned_vec(lin.to(DEV)), T, P, C, layer)
    f64, l64 = f.double(), lin.double()
    n = f64 / (f64.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    want = (((n[:T] - n[T:]) ** 2) * l64).sum(dim=(1, 2)).numpy()
    scale = ((n[:T] ** 2 + n[T:] ** 2) * l64).sum(dim=(1, 2)).numpy()
    tol = 4.0 * math.sqrt(C) * 2.0 ** -24 * scale
    ratio = np.abs(got - want) / tol
    print(f"distance P {P} C {C}: worst error / tolerance {ratio.max():.4f} (values {want})")
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), (got, want, ratio)
    zeros = torch.zeros(2 * T * P * C, dtype=torch.float32, device=DEV)
    assert _distance(zeros, lin.to(DEV), T, P, C, layer).tolist() == [0.0] * T               # every pixel all zero: 0, not NaN


E2E_TOL_REL = 4.0 * math.sqrt(3456) * 2.0 ** -24
_WORST = {"ratio": 0.0}


def _check_e2e(tag, ref_h, rec_h, got, rescale, model):
    """ref_h, rec_h: host [3,T,H,W] arrays holding exactly the values the GPU read"""
    v64, l64 = lpips_ref.video(ref_h, rec_h, model, rescale)
    v32, _ = lpips_ref.video(ref_h, rec_h, model, rescale, dtype=torch.float32)
    e32 = np.abs(v32 - v64)
    tol = np.maximum(16.0 * e32, E2E_TOL_REL * np.abs(v64))
    err = np.abs(np.asarray(got) - v64)
    ok = err <= tol
    ratio = float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0
    _WORST["ratio"] = max(_WORST["ratio"], ratio)
    print(f"{tag}: LPIPS {v64} per-layer {l64[0]} e32 {e32.max():.2e} |gpu - fp64| {err.max():.2e} worst error / tolerance {ratio:.3f} "
          f"(so far {_WORST['ratio']:.3f})")
    assert got.dtype == np.float64 and ok.all(), (tag, got, v64, err, tol)
    return v64


E2E_CASES = [
    # tag, dtype, rescale, layout, shape, noise
    ("f16-rescale-0.1", torch.float16, True, "contiguous", (3, 2, 34, 47), 0.1),
    ("f32-rescale-0.5", torch.float32, True, "contiguous", (3, 2, 38, 43), 0.5),
    ("f16-unit-0.5", torch.float16, False, "contiguous", (3, 2, 31, 35), 0.5),
    ("f32-unit-0.1", torch.float32, False, "contiguous", (3, 2, 34, 47), 0.1),
    ("f16-t-strided", torch.float16, True, "t", (3, 3, 31, 31), 0.1),
    ("f32-t-strided", torch.float32, True, "t", (3, 2, 38, 43), 0.1),
    ("f16-h-strided", torch.float16, True, "h", (3, 2, 34, 47), 0.5),
    ("f32-h-strided", torch.float32, True, "h", (3, 2, 31, 35), 0.1),
    ("f16-90x160", torch.float16, True, "contiguous", (3, 3, 90, 160), 0.1),
]


@pytest.mark.parametrize("tag,dtype,rescale,layout,shape,noise", E2E_CASES, ids=[c[0] for c in E2E_CASES])
def test_end_to_end_against_float64_restatement(tag, dtype, rescale, layout, shape, noise):
    model = _model()
    a, b = _pair(shape, "lpips.e2e." + tag, noise, unit=not rescale)
    ref, rec = _strided(a.to(DEV, dtype), layout), _strided(b.to(DEV, dtype), layout)
    got, layers = metrics.lpips_video(ref, rec, model, rescale=rescale, return_layers=True)
    assert got.shape == (shape[1],) and layers.shape == (shape[1], 5) and (layers > 0).all()
    _check_e2e(tag, a.float().numpy(), b.float().numpy(), got, rescale, model)


def test_batch_unequal_frame_counts_and_video_metrics_wiring():
    model = _model()
    pairs = [_pair((3, 3, 34, 47), f"lpips.batch.{i}", 0.1) for i in range(2)]
    a = torch.stack([p[0] for p in pairs]).to(DEV)
    b = torch.stack([p[1] for p in pairs]).to(DEV)[:, :, :2]                 # rec is one frame shorter: the common prefix is scored
    got = metrics.lpips_video(a, b, model)
    assert got.shape == (2, 2)
    for i in range(2):
        _check_e2e(f"batch row {i}", pairs[i][0].float().numpy(), pairs[i][1][:, :2].float().numpy(), got[i], True, model)
        assert np.array_equal(metrics.lpips_video(a[i], b[i], model), got[i])
    plain = metrics.video_metrics(a, b)
    m = metrics.video_metrics(a, b, lpips=model)
    assert "lpips" not in plain and np.array_equal(m["lpips"], got) and m["lpips_mean"] == float(got.mean())
    assert np.array_equal(m["psnr"], plain["psnr"]) and np.array_equal(m["ssim"], plain["ssim"])
    acc = metrics.MetricsAccumulator(lpips=model)
    acc.add_video(a, b)
    assert acc.frames == 4 and acc.result()["LPIPS"] == pytest.approx(float(got.mean()), abs=1e-15)


def test_identical_frame_is_zero_two_calls_agree_and_chunking_changes_no_bit():
    model = _model()
    a, b = _pair((3, 5, 38, 43), "lpips.exact", 0.1)
    b[:, 3] = a[:, 3]                                                        # one identical frame
    a, b = a.to(DEV), b.to(DEV)
    one, l1 = metrics.lpips_video(a, b, model, return_layers=True)
    two, l2 = metrics.lpips_video(a, b, model, return_layers=True)
    assert one[3] == 0.0 and not l1[3].any() and (np.delete(one, 3) > 0).all()
    assert np.array_equal(one, two) and np.array_equal(l1, l2)
    for fpc in (2, 1, 5):
        c, lc = metrics.lpips_video(a, b, model, frames_per_chunk=fpc, return_layers=True)
        assert np.array_equal(c, one) and np.array_equal(lc, l1), fpc


def test_bad_arguments_launch_nothing():
    model = _model()
    wts = model.on(DEV)
    ok = torch.zeros(3, 1, 31, 31, dtype=torch.float16, device=DEV)
    out = GuardedFlat(2 * 7 * 7 * 64, torch.float32)

    def conv1(v, H, W, dtype=0, rescale=1, T=1):
        _lib.call("lpips_conv1_f32", v, v.stride(0), v.stride(1), v.stride(2), v, v.stride(0), v.stride(1), v.stride(2), dtype, T, H, W,
                  rescale, wts["lut"], wts["w"][0], wts["b"][0], out.view)

    for v, H, W in ((ok[:, :, :30], 30, 31), (ok[:, :, :, :30], 31, 30)):    # H or W < 31
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            conv1(v, H, W)
    for kw in ({"dtype": 2}, {"rescale": 3}, {"T": 0}):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            conv1(ok, 31, 31, **kw)
    x = torch.zeros(2 * 3 * 3 * 64, dtype=torch.float32, device=DEV)
    for ci, co, k, pad in ((48, 192, 5, 2), (64, 100, 5, 2), (64, 192, 12, 2), (64, 192, 3, 3), (0, 64, 3, 1)):   # shapes no weight tensor has
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            _lib.call("lpips_conv2d_f32", x, wts["w"][1], wts["b"][1], out.view, 2, 3, 3, ci, co, k, pad)
    with pytest.raises(_lib.HVKernelError, match="bad argument"):
        _lib.call("lpips_maxpool_f32", x, out.view, 2, 2, 3, 64)             # H < 3
    with pytest.raises(_lib.HVKernelError, match="bad argument"):
        _lib.call("lpips_maxpool_f32", x, out.view, 2, 3, 3, 6)              # C % 4
    buf, o = _out_buffer(3)
    need = _lib.host("lpips_distance_workspace_bytes", 3, 819)
    assert need == 3 * 13 * 8 and _lib.host("lpips_distance_workspace_bytes", 0, 819) == 0
    ws = GuardedFlat(need, torch.uint8, front=16)
    f = torch.zeros(6 * 819 * 64, dtype=torch.float32, device=DEV)
    for args in ((3, 819, 64, 0, need - 8), (3, 819, 64, 5, need), (3, 819, 448, 0, need), (0, 819, 64, 0, need)):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            _lib.call("lpips_distance_f32", f, wts["lin"][0], args[0], args[1], args[2], args[3], o, ws.view, args[4])
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and bool((buf == 0x7F5A5A5A7F5A5A5A).all())
    assert bool((out.buf == out.sent).all()) and bool((ws.buf == ws.sent).all())
    small = torch.zeros(3, 2, 30, 40, dtype=torch.float16, device=DEV)
    with pytest.raises(_lib.HVKernelError, match="31"):
        metrics.lpips_video(small, small, model)
    with pytest.raises(_lib.HVKernelError):
        metrics.lpips_video(ok.bfloat16(), ok.bfloat16(), model)
    with pytest.raises(_lib.HVKernelError):
        metrics.lpips_video(ok[:1], ok[:1], model)                           # C = 1
    with pytest.raises(ValueError, match="layer 2"):
        LpipsAlex([(w, b) if i != 1 else (w[:, :32], b) for i, (w, b) in enumerate(model.convs)], model.lins)
    assert LPIPS_CHNS == (64, 192, 384, 256, 256)
