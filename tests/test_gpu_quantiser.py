"""GPU: quantise() of csrc/hv_common.hpp - the 8-bit frame value every scoring kernel reads its input through - value by value against
the fp32-stepwise utils.file_utils.frames_uint8 (tests/metrics_ref.quantise; the sets and what they cover: tests/metrics_bounds.py,
checked on the host by tests/test_metrics_bounds_cpu.py).

  * per element: hv_i3d_preprocess on a 224 x 224 clip returns (b / 255 - 0.5) * 2 bit for bit, an invertible read-out of the byte b of
    every cell: all 65,536 fp16 patterns, the +-8 ulp neighbourhood of every byte threshold in fp32, the specials, and NaNs (byte 0).
  * near per element: the same sets as 7 x 7 frames of a C = 1 video through hv_video_metrics against the set rotated by one position -
    sse and min / max are exact integers per 49 values (the kernel's smallest legal frame, a four-digit T).
  * aggregate, the other two readers on the same fp16 clip: bin 0 of the gray spectrum at T = 1 is the exact integer sum of the lumas
    (its power the sum of their squares); hv_lpips_conv1_f32 against the fp64 conv of the LUT values of the reference bytes under the
    bound of tests/test_gpu_lpips.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import _lib, metrics  # noqa: E402
from tests import metrics_bounds as MB  # noqa: E402
from tests.guarded_memory import GuardedFlat, same_bits  # noqa: E402

DEV = "cuda:0"
NP = {torch.float16: np.float16, torch.float32: np.float32}
_CLIPS = {}


def _clip(dtype, rescale):
    """(host clip [3,1,224,224] of `dtype`, its NaN cells, the reference bytes [3,1,224,224]) - once per (dtype, rescale)"""
    key = (dtype, rescale)
    if key not in _CLIPS:
        flat, cells = MB.clip_cells(MB.value_set(NP[dtype], rescale), MB.nans(NP[dtype]))
        want = MB.expected_bytes(flat, rescale)
        assert not want[cells].any() and len(np.unique(want)) == 256
        _CLIPS[key] = (torch.from_numpy(flat.reshape(MB.CLIP)), cells, want.reshape(MB.CLIP))
    return _CLIPS[key]


def _strided_h(x):
    """rows of a taller, wider buffer: row stride > W, an odd element offset (no 16-byte alignment)"""
    C, T, H, W = x.shape
    buf = torch.full((C, T, 2 * H + 1, W + 5), -0.5, dtype=x.dtype, device=x.device)
    buf[:, :, 1:2 * H:2, 3:3 + W] = x
    return buf[:, :, 1:2 * H:2, 3:3 + W]


@pytest.mark.parametrize("layout", ["contiguous", "h"])
@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_every_value_through_the_i3d_preprocess(dtype, rescale, layout):
    host, cells, want = _clip(dtype, rescale)
    dev = host.to(DEV)
    assert same_bits(dev.cpu(), host)                                                               # NaN payloads survive the copy
    dev = _strided_h(dev) if layout == "h" else dev
    out = GuardedFlat(224 * 224 * 4, torch.float32)
    _lib.call("i3d_preprocess", dev, dev.stride(0), dev.stride(1), dev.stride(2), 0 if dtype == torch.float16 else 1, 1, 224, 224, 224, 224,
              1 if rescale else 0, out.view)
    y = out.view.cpu().reshape(224, 224, 4)
    assert out.intact() and not y[..., 3].any() and torch.isfinite(y).all()
    y = y[..., :3].permute(2, 0, 1).contiguous()                                                    # [3, 224, 224]
    b = torch.round((y.double() / 2 + 0.5) * 255)
    assert float(b.min()) >= 0 and float(b.max()) <= 255
    assert same_bits(y, ((b.float() / 255.0) - 0.5) * 2)                                            # an exact read-out of the byte
    got = b.numpy().astype(np.uint8).reshape(-1)
    flat_want = want.reshape(-1)
    bad = np.flatnonzero(got != flat_want)
    x = host.reshape(-1).numpy()
    assert bad.size == 0, (f"{bad.size} cells differ; first: " +
                           ", ".join(f"x {float(x[i])!r} (bits {int(x[i:i + 1].view(np.uint16 if dtype == torch.float16 else np.uint32)[0]):#x}) "
                                     f"got {got[i]} want {flat_want[i]}" for i in bad[:8]))
    assert not got[cells].any()                                                                     # NaN quantises to 0


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_every_value_through_the_metrics_kernel_as_7x7_frames(dtype, rescale):
    vals = np.concatenate([MB.value_set(NP[dtype], rescale), MB.nans(NP[dtype])]) if dtype == torch.float32 else MB.fp16_all()
    a, b = MB.frames_7x7(vals), MB.frames_7x7(np.roll(vals, 1))
    T = a.shape[1]
    assert T == (1338 if dtype == torch.float16 else -(-len(vals) // 49)) and np.isnan(a.astype(np.float32)).any()
    ref = MB.Reference(a, b, rescale, ssim=False)
    st = metrics.video_stats(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), rescale)
    got = {"sse": st["sse"][0].cpu().numpy(), "minmax": st["minmax"][0].cpu().numpy()}
    assert got["sse"].shape == (T,) and len({tuple(m) for m in ref.minmax}) > 50
    MB.check_integers(got, ref, (dtype, rescale))
    assert torch.isfinite(st["ssim_sum"]).all()


@pytest.mark.parametrize("rescale", [True, False])
def test_gray_spectrum_dc_of_the_fp16_clip_is_the_exact_luma_sum(rescale):
    host, _, want = _clip(torch.float16, rescale)
    y = MB.luma(want[:, 0], metrics.GRAY_LUMA)                                                      # [224, 224] integers
    for dev in (host.to(DEV), _strided_h(host.to(DEV))):
        mag, pw, n = metrics.spectrum_sums(dev, mode="gray", rescale=rescale)
        assert n == 224 * 224 and tuple(mag.shape) == (1, 1)
        assert float(mag[0, 0]) == float(int(y.sum())) and float(pw[0, 0]) == float(int((y * y).sum()))
    assert int((y * y).sum()) < 2 ** 53 and len(np.unique(y)) > 100 and len(np.unique(want)) == 256


def test_lpips_first_conv_on_the_fp16_clip():
    """both images of the pair are the value sweep (the second rotated by one cell): the conv sees the byte of every fp16 pattern"""
    from tests import test_gpu_lpips as TL
    host, _, want = _clip(torch.float16, True)
    rot = torch.from_numpy(np.roll(host.numpy().reshape(-1), 1).reshape(MB.CLIP))
    want2 = MB.expected_bytes(rot.numpy(), True)
    model = TL._model()
    wts = model.on(DEV)
    va, vb = host.to(DEV), _strided_h(rot.to(DEV))
    out = GuardedFlat(2 * 55 * 55 * 64, torch.float32)
    _lib.call("lpips_conv1_f32", va, va.stride(0), va.stride(1), va.stride(2), vb, vb.stride(0), vb.stride(1), vb.stride(2), 0, 1, 224, 224,
              1, wts["lut"], wts["w"][0], wts["b"][0], out.view)
    lut = metrics.lpips_lut().double()
    qi = torch.from_numpy(np.concatenate([want, want2], axis=1)).long()                             # [3, 2, 224, 224]
    x = torch.stack([lut[c][qi[c]] for c in range(3)], dim=-1)                                      # [2, 224, 224, 3]
    ref, oh, ow = TL._conv_ref(x, model.convs[0][0], model.convs[0][1], 4, 2)
    assert (oh, ow) == (55, 55) and out.intact()
    TL._check_conv(out.view.reshape(2 * 55 * 55, 64), ref, "conv1 on the quantiser sweep")
