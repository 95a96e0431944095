"""Restatement of the reference's FVD inputs on torch CPU ops, in float64 or float32: the Inception-I3D network
(rebuttal/common_metrics_on_video_quality/fvd/videogpt/pytorch_i3d.py) and the preprocessing of fvd/videogpt/fvd.py:21-60.  It is pinned
to vectors made by executing the reference (tools/make_golden_i3d.py -> tests/golden/i3d_*.npz, tests/test_i3d_cpu.py) and is what the
GPU kernels of csrc/hv_i3d.hip are compared with (tests/test_gpu_i3d.py).  It walks the architecture on its own, from the state dict's
names - not through metrics.I3D_LAYERS, which it thereby checks."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from hunyuanvideo_efficiency_amd import synthetic as syn
from tests import metrics_ref

ENDPOINTS = ("Conv3d_1a_7x7", "MaxPool3d_2a_3x3", "Conv3d_2b_1x1", "Conv3d_2c_3x3", "MaxPool3d_3a_3x3", "Mixed_3b", "Mixed_3c",
             "MaxPool3d_4a_3x3", "Mixed_4b", "Mixed_4c", "Mixed_4d", "Mixed_4e", "Mixed_4f", "MaxPool3d_5a_2x2", "Mixed_5b", "Mixed_5c")
_POOLS = {"MaxPool3d_2a_3x3": ((1, 3, 3), (1, 2, 2)), "MaxPool3d_3a_3x3": ((1, 3, 3), (1, 2, 2)),
          "MaxPool3d_4a_3x3": ((3, 3, 3), (2, 2, 2)), "MaxPool3d_5a_2x2": ((2, 2, 2), (2, 2, 2))}
_CONVS = {"Conv3d_1a_7x7": ((7, 7, 7), (2, 2, 2)), "Conv3d_2b_1x1": ((1, 1, 1), (1, 1, 1)), "Conv3d_2c_3x3": ((3, 3, 3), (1, 1, 1))}


def same_pad(x, k, s):
    """zero padding of [N,C,T,H,W] by the rule of pytorch_i3d.py:9-33: per axis total = max(k - s, 0) if extent % s == 0 else
    max(k - extent % s, 0), front = total // 2"""
    pad = []
    for a in (2, 1, 0):                       # F.pad takes the last axis first
        e = x.shape[2 + a]
        total = max(k[a] - s[a], 0) if e % s[a] == 0 else max(k[a] - e % s[a], 0)
        pad += [total // 2, total - total // 2]
    return F.pad(x, pad)


def unit3d(x, sd, name, k, s):
    """Unit3D: pad, conv without bias, eval BatchNorm (eps 1e-5), ReLU"""
    g = lambda key: sd[f"{name}.{key}"].to(x.dtype)  # noqa: E731
    y = F.conv3d(same_pad(x, k, s), g("conv3d.weight"), None, stride=s)
    y = F.batch_norm(y, g("bn.running_mean"), g("bn.running_var"), g("bn.weight"), g("bn.bias"), False, 0.0, 1e-5)
    return F.relu(y)


def maxpool(x, k, s):
    return F.max_pool3d(same_pad(x, k, s), k, s)


def inception(x, sd, name):
    one, three = (1, 1, 1), (3, 3, 3)
    b0 = unit3d(x, sd, f"{name}.b0", one, one)
    b1 = unit3d(unit3d(x, sd, f"{name}.b1a", one, one), sd, f"{name}.b1b", three, one)
    b2 = unit3d(unit3d(x, sd, f"{name}.b2a", one, one), sd, f"{name}.b2b", three, one)
    b3 = unit3d(maxpool(x, three, one), sd, f"{name}.b3b", one, one)
    return torch.cat([b0, b1, b2, b3], dim=1)


def head(x, sd):
    """[1,1024,T',7,7] -> [400]: AvgPool3d([2,7,7], 1), the logits conv with bias, the mean over time"""
    y = F.avg_pool3d(x, (2, 7, 7), (1, 1, 1))
    y = F.conv3d(y, sd["logits.conv3d.weight"].to(x.dtype), sd["logits.conv3d.bias"].to(x.dtype))
    return y[0, :, :, 0, 0].mean(dim=1)


def network(x, sd, dtype=torch.float64, endpoints=False):
    """x [3,T,H,W] (host) -> logits [400] in `dtype`; with endpoints also {name: [C,T,H,W]}"""
    x = x.to(dtype)[None]
    eps = {}
    for ep in ENDPOINTS:
        if ep in _POOLS:
            x = maxpool(x, *_POOLS[ep])
        elif ep in _CONVS:
            x = unit3d(x, sd, ep, *_CONVS[ep])
        else:
            x = inception(x, sd, ep)
        if endpoints:
            eps[ep] = x[0]
    y = head(x, sd)
    return (y, eps) if endpoints else y


def channels_last4(x):
    """[3,T,H,W] -> the kernels' [T,H,W,4] fp32 with a zero fourth channel"""
    T, H, W = x.shape[1:]
    out = torch.zeros(T, H, W, 4, dtype=torch.float32)
    out[..., :3] = x.permute(1, 2, 3, 0)
    return out


def resized(H, W):
    """fvd.py:32-36"""
    scale = 224 / min(H, W)
    return (224, math.ceil(W * scale)) if H < W else (math.ceil(H * scale), 224)


def preprocess_bytes(b, dtype=torch.float32):
    """uint8 frames [3,T,H,W] -> [3,T,224,224] as fvd.py:21-60: / 255, bilinear resize of the shorter side to 224 (align_corners=False),
    centre crop, - 0.5, * 2"""
    v = torch.from_numpy(np.ascontiguousarray(b)).permute(1, 0, 2, 3).to(dtype) / 255.0                 # [T,3,H,W]
    v = F.interpolate(v, size=resized(*v.shape[2:]), mode="bilinear", align_corners=False)
    h0, w0 = (v.shape[2] - 224) // 2, (v.shape[3] - 224) // 2
    v = v[:, :, h0:h0 + 224, w0:w0 + 224].permute(1, 0, 2, 3).contiguous()
    return (v - 0.5) * 2


def preprocess(video, rescale=True, dtype=torch.float32):
    """[3,T,H,W] float video -> the bytes frames_uint8 writes of it, then preprocess_bytes"""
    return preprocess_bytes(metrics_ref.quantise(video.float().numpy(), rescale), dtype)


# ---- what tools/make_golden_i3d.py and the tests regenerate from seeds -----------------------------------------------------------------------
GOLDEN_INPUT = (3, 10, 200, 193)
GOLDEN_CLIPS = {"40x56": (3, 2, 40, 56), "57x41": (3, 2, 57, 41)}
GOLDEN_SAMPLES = 64


def golden_input():
    """the network input of the goldens, [3,10,200,193] in [-1, 1)"""
    return syn.hashed_uniform(GOLDEN_INPUT, "i3d.golden.input", 0)


def golden_bytes(tag):
    """a uint8 clip [3,T,H,W]: smooth ramps plus hashed noise, so that the resize has something to interpolate"""
    shape = GOLDEN_CLIPS[tag]
    _, T, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([40 + 150 * xx / (W - 1), 220 - 170 * yy / (H - 1), 60 + 120 * (xx + yy) / (H + W - 2)])[:, None]
    noise = 30 * syn.hashed_uniform(shape, "i3d.golden.clip." + tag, 0)
    return (base + noise).clamp(0, 255).floor().to(torch.uint8).numpy()


def sample_index(n, key, count=GOLDEN_SAMPLES):
    """`count` flat indices into a tensor of n elements, a pure function of (n, key)"""
    u = syn.hashed_uniform((count,), "i3d.golden.sample." + key, 0).double()
    return ((u + 1.0) / 2.0 * n).long().clamp(0, n - 1)


def golden_features(n, d, key, shift=0.0):
    """a seeded feature set [n, d] float64 with correlated columns"""
    z = syn.hashed_uniform((n, d), "i3d.golden.feat." + key, 0).double()
    mix = syn.hashed_uniform((d, d), "i3d.golden.mix." + key, 0).double() / math.sqrt(d)
    return (z @ mix + 0.5 * z + shift).numpy()


FRECHET_CASES = (("n6_d400", 6, 400, 0.1), ("n24_d8", 24, 8, 0.3), ("n1_d400", 1, 400, 0.2), ("n40_d16", 40, 16, 0.0))
