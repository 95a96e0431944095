"""GPU: the I3D kernels of csrc/hv_i3d.hip through the C ABI one by one, and metrics.i3d_logits / fvd_logits / MetricsAccumulator(fvd=)
end to end, against the restatement tests/i3d_ref.py (itself pinned to the executed reference by tests/test_i3d_cpu.py).  Operands sit
in NaN-poisoned buffers, outputs in sentinel-guarded ones (tests/guarded_memory.py).

Bounds.
  * conv: element by element against the fp64 conv of the same operands under tests/error_bounds.py (one Ref.add per tap with the
    folded scale multiplied into the weights, the shift as bias, bound(torch.float32)): the MFMA is an fp32 fma chain, the model that
    bound assumes; ReLU is 1-Lipschitz, so |relu(got) - relu(y64)| obeys the bound of y64.
  * max pool: exact against the restatement (F.pad with zeros, then max_pool3d).
  * head, stage by stage with the plain fp32-chain bound.  The pooled values the kernel left in its workspace against fp64: a chain of
    98 terms x / 98.  Each time position's logits against fp64 ON THOSE fp32 pooled values: a chain of 1024, with the bias.  The output
    against the mean of those: the bound of a position holds 2^-23 |y_t|, of which the rounding of acc + bias uses half; the mean of the
    other halves, 2^-24 mean |y_t| >= 2^-24 |y|, is the one rounding of the two-term sum (T' = 3; the division by 2 is exact, and for
    T' = 2 the mean is the identity).  So |got - mean_t y_t| <= mean_t bound_t, nothing added.
  * preprocessing: |got - F.interpolate pipeline| <= 8 * 2^-24 on the [-1, 1] output: the source coordinates are identical by
    construction (one fma), the blend is four fp32 roundings per side of values <= 1, doubled by the final * 2.  A 224 x 224 clip has
    integer coordinates and weights (1, 0): bit-exact (b / 255 - 0.5) * 2.
  * whole network: per logit |GPU - fp64 restatement| <= 16 * e32, e32 = max |fp32 restatement - fp64 restatement| on the same input;
    16 covers the MFMA's strictly k-ordered chains against the CPU's blocked sums."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _lib, metrics  # noqa: E402
from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402
from hunyuanvideo_efficiency_amd.metrics import I3D, MetricsAccumulator, frechet_distance  # noqa: E402
from tests import error_bounds as eb  # noqa: E402
from tests import i3d_ref, metrics_ref  # noqa: E402
from tests.guarded_memory import INT, NAN_BITS, Guarded, GuardedFlat, poisoned_vec, same_bits  # noqa: E402

DEV = "cuda:0"
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        _CACHE["model"] = I3D.synthetic(0)
    return _CACHE["model"]


class PoisonedSlice:
    """rows [M, C] at columns [c0, c0 + C) of a NaN-filled fp32 buffer [before + M + after][c0 + C + pad]; the view's first element is
    16-byte aligned (c0 and the pitch are multiples of 4)"""

    def __init__(self, t, c0=0, pad=0, before=3, after=5):
        M, C = t.shape
        self.pitch = c0 + C + pad
        assert c0 % 4 == 0 and self.pitch % 4 == 0
        self.buf = torch.full((before + M + after, self.pitch), NAN_BITS[4], dtype=INT[4], device=DEV)
        self.view = self.buf.view(torch.float32)[before:before + M, c0:c0 + C]
        self.view.copy_(t)


def _taps_ref(x_cl, w, sc, sh, k, s, pads):
    """x_cl [T,H,W,Cin] fp64 (host), w [Cout,Cin,kt,kh,kw], folded sc / sh -> (error_bounds.Ref over output rows, output extents)"""
    T, H, W, Cin = x_cl.shape
    out = tuple(-(-e // st) for e, st in zip((T, H, W), s))
    size = [max(pads[a] + (T, H, W)[a], (out[a] - 1) * s[a] + k[a]) for a in range(3)]
    xp = torch.zeros(*size, Cin, dtype=torch.float64)
    xp[pads[0]:pads[0] + T, pads[1]:pads[1] + H, pads[2]:pads[2] + W] = x_cl
    ws = w.double() * sc.double()[:, None, None, None, None]
    ref = eb.Ref()
    for dt in range(k[0]):
        for dh in range(k[1]):
            for dw in range(k[2]):
                a = xp[dt:dt + s[0] * (out[0] - 1) + 1:s[0], dh:dh + s[1] * (out[1] - 1) + 1:s[1], dw:dw + s[2] * (out[2] - 1) + 1:s[2]]
                ref.add(a.reshape(-1, Cin), ws[:, :, dt, dh, dw])
    return ref.bias(sh), out


CONV_CASES = [
    # tag, kernel, stride, extents (T, H, W), Cin, Cout, relu, (input c0, pad), (output c0, pad)
    ("k7s2-T<k-even|odd", 7, 2, (3, 18, 15), 16, 16, 1, (0, 0), (0, 0)),           # T shorter than the kernel; pads 2 | 3 (18) and 3 | 3 (15)
    ("k7s2-first-layer", 7, 2, (10, 15, 18), 4, 64, 1, (0, 0), (0, 0)),            # the 4-channel input: 8 taps per 32-wide k chunk
    ("k7s2-24-slices", 7, 2, (10, 15, 18), 24, 24, 0, (8, 12), (8, 16)),           # a chunk straddles taps (24 does not divide 32)
    ("k3-one-voxel", 3, 1, (1, 1, 1), 112, 208, 1, (4, 4), (0, 0)),                # every tap but the centre is padding; 208 = 3 * 64 + 16
    ("k3-2x7x7", 3, 1, (2, 7, 7), 528, 400, 0, (0, 0), (16, 8)),                   # the logits width: 400 = 6 * 64 + 16
    ("k3-M129", 3, 1, (1, 3, 43), 16, 24, 1, (0, 0), (0, 0)),                      # the last tile holds 1 row
    ("k3-M255", 3, 1, (3, 5, 17), 24, 16, 1, (16, 8), (4, 0)),                     # the last tile holds 127 rows
    ("k1-528", 1, 1, (2, 7, 7), 528, 16, 1, (0, 0), (8, 16)),
    ("k1-112-slices", 1, 1, (3, 5, 17), 112, 208, 0, (8, 8), (8, 16)),
    # per-axis extents and strides: a swap of kh and kw, or of two strides, shows here
    ("k133-s122", (1, 3, 3), (1, 2, 2), (3, 9, 14), 16, 24, 1, (0, 0), (0, 0)),
    ("k317-s212", (3, 1, 7), (2, 1, 2), (5, 6, 11), 24, 16, 0, (8, 8), (4, 8)),
    ("k731-s121", (7, 3, 1), (1, 2, 1), (4, 7, 5), 16, 16, 1, (0, 0), (0, 0)),
]


@pytest.mark.parametrize("tag,k,s,ext,ci,co,relu,xs,ys", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_alone_against_fp64(tag, k, s, ext, ci, co, relu, xs, ys):
    T, H, W = ext
    kk, ss = ((k, k, k), (s, s, s)) if isinstance(k, int) else (k, s)
    pads, out = zip(*(metrics.i3d_same_pad(kk[a], ss[a], ext[a]) for a in range(3)))
    x = syn.hashed_uniform((T * H * W, ci), f"i3d.conv.x.{tag}", 0)
    w = syn.hashed_uniform((co, ci, *kk), f"i3d.conv.w.{tag}", 0) * math.sqrt(6.0 / (ci * kk[0] * kk[1] * kk[2]))
    sc = 1.0 + 0.2 * syn.hashed_uniform((co,), f"i3d.conv.sc.{tag}", 0)
    sh = 0.1 * syn.hashed_uniform((co,), f"i3d.conv.sh.{tag}", 0)
    xin = PoisonedSlice(x, *xs)
    M = out[0] * out[1] * out[2]
    y = Guarded(M, co, torch.float32, c0=ys[0], pad=ys[1])
    _lib.call("i3d_conv3d_f32", xin.view, xin.pitch, poisoned_vec(metrics.i3d_pack_conv(w).reshape(-1).to(DEV)), poisoned_vec(sc.to(DEV)),
              poisoned_vec(sh.to(DEV)), y.view, y.buf.shape[1], T, H, W, ci, co, *kk, *ss, *pads, relu)
    ref, out_ref = _taps_ref(x.double().reshape(T, H, W, ci), w, sc, sh, kk, ss, pads)
    assert out_ref == tuple(out) and ref.y.shape == (M, co)
    assert y.intact(), f"{tag}: wrote outside its column slice"
    g = y.view.double().cpu()
    want = ref.y.clamp(min=0.0) if relu else ref.y
    r = (g - want).abs() / ref.bound(torch.float32)
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, math.inf))
    live = float((g > 0).double().mean())
    print(f"conv {tag}: K {ref.k} rows {M} worst error / bound {float(r.max()):.3f}, positive outputs {live:.2f}")
    assert float(r.max()) <= 1.0, f"{tag}: {int((r > 1).sum())} of {r.numel()} elements outside the fp64 bound (worst {float(r.max()):.3g})"
    assert 0.1 < live < 0.9, (tag, live)


POOL_CASES = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((2, 2, 2), (2, 2, 2))]


@pytest.mark.parametrize("k,s", POOL_CASES, ids=["1x3x3-s122", "3x3x3-s2", "3x3x3-s1", "2x2x2-s2"])
@pytest.mark.parametrize("ext,C", [((3, 7, 9), 24), ((4, 8, 6), 64), ((1, 1, 1), 4), ((5, 13, 12), 208)])
def test_maxpool_exact_and_zero_padding_takes_part(k, s, ext, C):
    T, H, W = ext
    pads, out = zip(*(metrics.i3d_same_pad(k[a], s[a], ext[a]) for a in range(3)))
    M = out[0] * out[1] * out[2]
    for kind in ("signed", "negative"):
        x = syn.hashed_uniform((T * H * W, C), f"i3d.pool.{k}.{s}.{ext}.{C}", 0)
        if kind == "negative":
            x = -x.abs() - 0.25
        xin = PoisonedSlice(x, 8, 4)
        y = Guarded(M, C, torch.float32, c0=8, pad=16)
        _lib.call("i3d_maxpool3d_f32", xin.view, xin.pitch, y.view, y.buf.shape[1], T, H, W, C, *k, *s, *pads)
        want = i3d_ref.maxpool(x.reshape(T, H, W, C).permute(3, 0, 1, 2)[None], k, s)[0].permute(1, 2, 3, 0).reshape(M, C)
        assert y.intact() and torch.equal(y.view.cpu(), want), (kind, k, s, ext, C)
        if kind == "negative":
            got = y.view.cpu().reshape(*out, C)
            padded = any(p > 0 for p in pads) or any((o - 1) * st + kk > e for o, st, kk, e in zip(out, s, k, ext))
            assert float(got.max()) == (0.0 if padded else float(x.max()))
            if pads[1] > 0:
                assert not got[:, 0].any()                      # a border window holds a padded zero: its maximum is 0, not negative
            if all(e > 2 for e in ext) and k == (3, 3, 3) and s == (1, 1, 1):
                assert float(got[1:-1, 1:-1, 1:-1].max()) < 0  # interior windows see no padding
    # a NaN cell makes exactly the windows that hold it NaN, as max_pool3d does
    x = syn.hashed_uniform((T * H * W, C), f"i3d.pool.nan.{k}.{s}.{ext}.{C}", 0)
    x[(T * H * W) // 2, 1] = float("nan")
    xin = PoisonedSlice(x, 8, 4)
    y = Guarded(M, C, torch.float32, c0=8, pad=16)
    _lib.call("i3d_maxpool3d_f32", xin.view, xin.pitch, y.view, y.buf.shape[1], T, H, W, C, *k, *s, *pads)
    want = i3d_ref.maxpool(x.reshape(T, H, W, C).permute(3, 0, 1, 2)[None], k, s)[0].permute(1, 2, 3, 0).reshape(M, C)
    got = y.view.cpu()
    assert y.intact() and bool(want.isnan().any()) and torch.equal(got.isnan(), want.isnan())
    assert torch.equal(got[~want.isnan()], want[~want.isnan()])


@pytest.mark.parametrize("T", [2, 3])
def test_head_against_fp64(T):
    model = _model()
    x = syn.hashed_uniform((T * 49, 1024), f"i3d.head.{T}", 0).clamp(min=0.0)                   # post-ReLU-like
    w = model.sd["logits.conv3d.weight"].reshape(400, 1024)
    b = model.sd["logits.conv3d.bias"]
    xin = PoisonedSlice(x, 8, 8)
    out = GuardedFlat(400, torch.float32)
    ws = GuardedFlat((T - 1) * 1024, torch.float32)
    _lib.call("i3d_head_f32", xin.view, xin.pitch, poisoned_vec(w.T.contiguous().reshape(-1).to(DEV)), poisoned_vec(b.to(DEV)), out.view,
              T, 7, 7, 1024, ws.view, (T - 1) * 1024)
    # stage 1: the pooled values in the workspace, each a 98-term chain of x / 98
    cells = torch.stack([x.double().reshape(T, 49, 1024)[t:t + 2].reshape(98, 1024).T for t in range(T - 1)]).reshape(-1, 98)
    pool_ref = eb.Ref().add(cells, torch.full((1, 98), 1.0 / 98.0, dtype=torch.float64))
    pooled = ws.view.cpu().reshape(-1, 1)                                                        # [(T - 1) * 1024, 1] fp32, the GPU's own
    rp = float(eb.ratio(pooled, pool_ref, torch.float32).max())
    # stage 2: every time position's logits on those fp32 pooled values, a 1024-term chain with the bias; the output is their mean
    refs = [eb.Ref().add(pooled.reshape(T - 1, 1024)[t:t + 1], w).bias(b) for t in range(T - 1)]
    y64 = torch.stack([r.y for r in refs]).mean(0)
    bound = torch.stack([r.bound(torch.float32) for r in refs]).mean(0)
    got = out.view.double().cpu().reshape(1, 400)
    r = (got - y64).abs() / bound
    want_ref = i3d_ref.head(x.double().reshape(T, 7, 7, 1024).permute(3, 0, 1, 2)[None], {k: v.double() for k, v in model.sd.items()})
    assert float((y64[0] - want_ref).abs().max()) <= 1e-5 * float(want_ref.abs().max())            # the staged value is the restatement's head
    print(f"head T' {T}: pooled worst error / bound {rp:.3f}, logits worst error / bound {float(r.max()):.3f}, logits up to "
          f"{float(y64.abs().max()):.2f}")
    assert out.intact() and ws.intact() and torch.isfinite(got).all() and rp <= 1.0 and float(r.max()) <= 1.0


def _clip(shape, key, dtype, unit=False):
    x = syn.hashed_uniform(shape, key, 0)
    # smooth content plus noise: neighbouring pixels differ, so a wrong interpolation weight shows
    C, T, H, W = shape
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    x = 0.6 * torch.stack([xx, yy, -0.5 * (xx + yy)])[:, None] + 0.4 * x
    x = (x + 1) / 2 if unit else x
    return x.to(dtype)


def _strided_h(x):
    """rows of a taller, wider NaN-free buffer: row stride > W, an odd element offset (tests/test_gpu_metrics.py's `h` layout)"""
    C, T, H, W = x.shape
    buf = torch.full((C, T, 2 * H + 1, W + 5), -0.5, dtype=x.dtype, device=x.device)
    buf[:, :, 1:2 * H:2, 3:3 + W] = x
    return buf[:, :, 1:2 * H:2, 3:3 + W]


PRE_CASES = [
    ("40x56-f16", (3, 2, 40, 56), torch.float16, True, False), ("57x41-f32", (3, 2, 57, 41), torch.float32, True, False),
    ("240x416-f16", (3, 2, 240, 416), torch.float16, True, False), ("40x56-f32-unit-strided", (3, 2, 40, 56), torch.float32, False, True),
    ("57x41-f16-unit", (3, 2, 57, 41), torch.float16, False, False), ("240x416-f32-strided", (3, 1, 240, 416), torch.float32, True, True),
    # square and not 224: the reference's ceil(200 * (224 / 200)) is 225, so the clip is resized to 225 x 224 and row 0 is the crop
    ("200x200-f16", (3, 2, 200, 200), torch.float16, True, False), ("100x100-f32-strided", (3, 2, 100, 100), torch.float32, False, True),
    ("150x150-f16", (3, 2, 150, 150), torch.float16, True, False),                                  # a square that resizes to 224 x 224
]


@pytest.mark.parametrize("tag,shape,dtype,rescale,strided", PRE_CASES, ids=[c[0] for c in PRE_CASES])
def test_preprocess_against_interpolate(tag, shape, dtype, rescale, strided):
    host = _clip(shape, "i3d.pre." + tag, dtype, unit=not rescale)
    dev = host.to(DEV)
    dev = _strided_h(dev) if strided else dev
    T = shape[1]
    RH, RW = metrics.i3d_resized(shape[2], shape[3])
    out = GuardedFlat(T * 224 * 224 * 4, torch.float32)
    _lib.call("i3d_preprocess", dev, dev.stride(0), dev.stride(1), dev.stride(2), 0 if dtype == torch.float16 else 1, T, shape[2], shape[3],
              RH, RW, 1 if rescale else 0, out.view)
    got = out.view.cpu().reshape(T, 224, 224, 4)
    want = i3d_ref.preprocess(host, rescale).permute(1, 2, 3, 0)                                   # [T,224,224,3] fp32, F.interpolate
    err = float((got[..., :3].double() - want.double()).abs().max()) / 2.0 ** -24
    print(f"preprocess {tag}: resized {RH} x {RW}, worst |got - torch| {err:.2f} units of 2^-24")
    assert out.intact() and not got[..., 3].any() and torch.isfinite(got).all()
    assert err <= 8.0 and float(want.std()) > 0.2
    assert same_bits(metrics.fvd_preprocess(dev, rescale), out.view.reshape(T, 224, 224, 4))       # the host wrapper makes this call


@pytest.mark.parametrize("dtype,rescale", [(torch.float16, True), (torch.float32, False)])
def test_preprocess_of_a_224_clip_is_the_bytes_bit_for_bit(dtype, rescale):
    host = _clip((3, 2, 224, 224), "i3d.pre.224", dtype, unit=not rescale)
    got = metrics.fvd_preprocess(host.to(DEV), rescale).cpu()
    b = torch.from_numpy(metrics_ref.quantise(host.float().numpy(), rescale)).float()              # [3,T,224,224]
    want = ((b / 255.0) - 0.5) * 2
    assert torch.equal(got[..., :3], want.permute(1, 2, 3, 0)) and not got[..., 3].any() and len(b.unique()) > 200


def test_every_clip_size_the_reference_accepts_is_accepted():
    """the resized extents of the reference's own arithmetic pass the kernel's argument check, squares whose ceil lands on 225 included"""
    seen = set()
    for H, W in ((40, 56), (57, 41), (240, 416), (720, 1280), (224, 224), (193, 200), (7, 1000), (1000, 7), (100, 100), (200, 200),
                 (400, 400), (25, 25), (50, 50), (164, 164), (150, 150), (1, 1)):
        clip = torch.zeros(3, 1, H, W, dtype=torch.float16, device=DEV)
        y = metrics.fvd_preprocess(clip)
        seen.add(metrics.i3d_resized(H, W)[0] - 224 if H == W else -1)
        flat = (127.0 / 255.0 - 0.5) * 2.0                        # a zero clip is byte 127 everywhere; the blend of a constant is the constant
        assert tuple(y.shape) == (1, 224, 224, 4) and not y[..., 3].any(), (H, W)
        assert float((y[..., :3].double() - flat).abs().max()) <= 8 * 2.0 ** -24, (H, W)
    assert {0, 1, -1} <= seen


def _network_refs(key, x):
    """fp64 and fp32 restatement logits of the network input x [3,T,H,W] (host), once per key"""
    if key not in _CACHE:
        sd = _model().state_dict()
        l64, l32 = i3d_ref.network(x, sd, torch.float64), i3d_ref.network(x, sd, torch.float32)
        _CACHE[key] = (l64, float((l32.double() - l64).abs().max()))
    return _CACHE[key]


def _check_logits(tag, got, l64, e32):
    err = (got.double().cpu() - l64).abs()
    tol = 16.0 * e32
    print(f"{tag}: logits std {float(l64.std()):.2f} max {float(l64.abs().max()):.2f}, e32 {e32:.3e}, worst |gpu - fp64| {float(err.max()):.3e}, "
          f"worst error / tolerance {float(err.max()) / tol:.3f}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (400,) and torch.isfinite(got).all()
    assert float(err.max()) <= tol, (tag, float(err.max()), tol)


def _fvd_clip(i=0, T=10, dtype=torch.float16):
    return _clip((3, T, 48, 64), f"i3d.e2e.clip{i}", dtype)


def test_network_alone_on_the_golden_input_non_square():
    x = i3d_ref.golden_input()                                                                     # [3,10,200,193]
    l64, e32 = _network_refs("golden", x)
    got = metrics.i3d_logits(i3d_ref.channels_last4(x).to(DEV), _model())
    _check_logits("i3d_logits 10x200x193", got, l64, e32)
    again = metrics.i3d_logits(i3d_ref.channels_last4(x).to(DEV), _model())
    assert same_bits(got, again)                                                                   # two runs: the same bits
    noisy = i3d_ref.channels_last4(x + 0.1 * syn.hashed_uniform(tuple(x.shape), "i3d.e2e.noise", 0)).to(DEV)
    moved = float((metrics.i3d_logits(noisy, _model()) - got).abs().max())
    assert moved > 100 * 16.0 * e32, moved                                                         # the tolerance is far below what an input change does


def test_fvd_logits_through_the_preprocessing_batches_and_short_clips():
    model = _model()
    clips = [_fvd_clip(i) for i in range(2)]
    x = i3d_ref.preprocess(clips[0], True)                                                         # [3,10,224,224] fp32, torch's resize
    l64, e32 = _network_refs("clip0", x)
    one = metrics.fvd_logits(clips[0].to(DEV), model)
    _check_logits("fvd_logits 10x48x64", one, l64, e32)
    batch = metrics.fvd_logits(torch.stack(clips).to(DEV), model)
    assert tuple(batch.shape) == (2, 400)
    for i in range(2):
        assert same_bits(batch[i], metrics.fvd_logits(clips[i].to(DEV), model)), i                 # clip i of a batch = its single run
    assert same_bits(batch[0], one) and not torch.equal(batch[0], batch[1])
    with pytest.raises(ValueError, match="10"):
        metrics.fvd_logits(clips[0][:, :9].to(DEV), model)
    with pytest.raises(_lib.HVKernelError):
        metrics.fvd_logits(clips[0][:2].to(DEV), model)                                            # C = 2
    with pytest.raises(_lib.HVKernelError):
        metrics.i3d_logits(torch.zeros(10, 192, 224, 4, device=DEV), model)                        # the last map would be 6 x 7


def test_accumulator_fvd_is_the_frechet_distance_of_its_logits():
    model = _model()
    refs = [_fvd_clip(i) for i in range(3)]
    recs = [(r.float() + 0.2 * syn.hashed_uniform(tuple(r.shape), f"i3d.acc.noise{i}", 0)).clamp(-1, 1).half() for i, r in enumerate(refs)]
    acc = MetricsAccumulator(fvd=model)
    m = acc.add_video(refs[0].to(DEV), recs[0].to(DEV))
    assert "FVD" not in acc.result() and acc.clips == 1 and tuple(m["fvd_ref_logits"].shape) == (400,)          # one clip: no FVD
    acc.add_video(torch.stack(refs[1:]).to(DEV), torch.stack(recs[1:]).to(DEV))
    lr = torch.stack([metrics.fvd_logits(r.to(DEV), model) for r in refs]).cpu().numpy()
    lc = torch.stack([metrics.fvd_logits(r.to(DEV), model) for r in recs]).cpu().numpy()
    res = acc.result()
    assert acc.clips == 3 and res["FVD"] == frechet_distance(lr, lc) and res["FVD"] > 0 and "PSNR" in res
    with pytest.raises(ValueError, match="10 frames"):                                             # a short pair is an error, and scores nothing
        acc.add_video(refs[0][:, :9].to(DEV), recs[0][:, :9].to(DEV))
    assert acc.clips == 3 and acc.frames == 30
    reuse = MetricsAccumulator(fvd=model)                                                          # the study's reuse of the inputs' logits
    for i in range(3):
        reuse.add_video(refs[i].to(DEV), recs[i].to(DEV), ref_logits=torch.from_numpy(lr[i]))
    assert reuse.result()["FVD"] == res["FVD"]
    print(f"FVD of 3 clip pairs under synthetic weights: {res['FVD']:.4f}")


def test_bad_arguments_launch_nothing():
    x = torch.zeros(4 * 7 * 7 * 1024 + 8, dtype=torch.float32, device=DEV)
    w = torch.zeros(27 * 1024 * 64, dtype=torch.float32, device=DEV)
    v = torch.zeros(1024, dtype=torch.float32, device=DEV)
    out = GuardedFlat(4 * 7 * 7 * 1024, torch.float32)

    def conv(xp=x, ldx=16, ldy=16, T=2, H=7, W=7, ci=16, co=16, k=(3, 3, 3), s=(1, 1, 1), p=(1, 1, 1), relu=1):
        _lib.call("i3d_conv3d_f32", xp, ldx, w, v, v, out.view, ldy, T, H, W, ci, co, *k, *s, *p, relu)

    for kw in ({"ci": 6}, {"co": 6}, {"ci": 0}, {"co": 4100}, {"k": (5, 3, 3)}, {"k": (3, 3, 2)}, {"s": (3, 1, 1)}, {"s": (1, 0, 1)},
               {"p": (3, 1, 1)}, {"p": (1, -1, 1)}, {"ldx": 12}, {"ldx": 18}, {"ldy": 12}, {"relu": 2}, {"T": 0}, {"xp": x[1:]}):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            conv(**kw)

    def pool(xp=x, ldx=16, ldy=16, C=16, k=(3, 3, 3), s=(2, 2, 2), p=(0, 1, 1)):
        _lib.call("i3d_maxpool3d_f32", xp, ldx, out.view, ldy, 2, 7, 7, C, *k, *s, *p)

    for kw in ({"C": 6}, {"k": (4, 3, 3)}, {"s": (3, 2, 2)}, {"p": (0, 3, 1)}, {"ldx": 12}, {"ldy": 18}, {"xp": x[2:]}):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            pool(**kw)

    ws = GuardedFlat(3 * 1024, torch.float32)

    def head(T=4, H=7, W=7, C=1024, ldx=1024, n=3 * 1024):
        _lib.call("i3d_head_f32", x, ldx, w, v, out.view, T, H, W, C, ws.view, n)

    for kw in ({"T": 1}, {"H": 6}, {"W": 8}, {"C": 512}, {"ldx": 1000}, {"n": 3 * 1024 - 1}, {"T": metrics._abi.MACROS["HV_I3D_HEAD_MAX_T"] + 1}):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            head(**kw)

    clip = torch.zeros(3, 2, 40, 56, dtype=torch.float16, device=DEV)

    def pre(dtype=0, RH=224, RW=314, rescale=1, T=2, sh=56):
        _lib.call("i3d_preprocess", clip, clip.stride(0), clip.stride(1), sh, dtype, T, 40, 56, RH, RW, rescale, out.view)

    for kw in ({"dtype": 2}, {"rescale": 2}, {"RH": 225}, {"RW": 223}, {"RH": 160, "RW": 224}, {"T": 0}, {"sh": 55}):
        with pytest.raises(_lib.HVKernelError, match="bad argument"):
            pre(**kw)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact() and bool((out.buf == out.sent).all()) and bool((ws.buf == ws.sent).all())
