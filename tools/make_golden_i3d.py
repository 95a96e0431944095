#!/usr/bin/env python3
"""Generate tests/golden/i3d_net.npz, i3d_preprocess.npz and i3d_frechet.npz by EXECUTING the reference's FVD code
(rebuttal/common_metrics_on_video_quality/fvd/videogpt/pytorch_i3d.py and fvd.py, loaded by path; nothing of them is copied):

  i3d_net         InceptionI3d(400, in_channels=3).eval() in fp32 under the I3D.synthetic(0) state dict on the seeded 10 x 200 x 193 input
                  of tests/i3d_ref.golden_input(): the 400 logits and 64 sampled values of each of the 16 endpoints (the sample positions
                  are tests/i3d_ref.sample_index, a pure function of the endpoint's size and name)
  i3d_preprocess  fvd.preprocess on the two byte clips of tests/i3d_ref.golden_bytes (40 x 56: H < W, 57 x 41: H > W), 2048 sampled
                  outputs each
  i3d_frechet     fvd.frechet_distance in fp64 on the seeded feature sets of tests/i3d_ref.FRECHET_CASES; the sets themselves are stored
                  (they are small) beside the distances

Inputs are regenerated from seeds by the tests, not stored.  Needs torch and einops (fvd.py imports it).
Run:  python tools/make_golden_i3d.py <reference root>"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hunyuanvideo_efficiency_amd.metrics import I3D  # noqa: E402
from tests import i3d_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PRE_SAMPLES = 2048


def load(ref_root, name):
    path = os.path.join(ref_root, "rebuttal", "common_metrics_on_video_quality", "fvd", "videogpt", name + ".py")
    spec = importlib.util.spec_from_file_location("ref_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: make_golden_i3d.py <root of the reference checkout>")
    net_mod, fvd_mod = load(sys.argv[1], "pytorch_i3d"), load(sys.argv[1], "fvd")
    torch.manual_seed(0)

    # ---- network
    model = net_mod.InceptionI3d(400, in_channels=3).eval()
    missing, unexpected = model.load_state_dict(I3D.synthetic(0).state_dict(), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    x = i3d_ref.golden_input()[None]
    out = {}
    with torch.no_grad():
        h = x
        for ep in model.VALID_ENDPOINTS:
            if ep in model.end_points:
                h = model._modules[ep](h)
                flat = h[0].reshape(-1)
                out["ep_" + ep] = flat[i3d_ref.sample_index(flat.numel(), ep)].numpy()
                out["shape_" + ep] = np.array(h.shape[1:])
                print(f"{ep:18s} {tuple(h.shape[1:])} live {float((h > 0).float().mean()):.2f}")
        logits = model(x)[0]
    out["logits"] = logits.numpy()
    print(f"logits: mean {float(logits.mean()):+.3f} std {float(logits.std()):.3f} max |.| {float(logits.abs().max()):.3f}")
    np.savez_compressed(os.path.join(GOLDEN, "i3d_net.npz"), **out)

    # ---- preprocessing: fvd.preprocess takes [B,C,T,H,W] floats in [0, 1] and truncates (v * 255) to bytes; (b + 0.5) / 255 lands on b
    out = {}
    for tag in i3d_ref.GOLDEN_CLIPS:
        b = i3d_ref.golden_bytes(tag)
        v = ((torch.from_numpy(b).float() + 0.5) / 255.0)[None]
        assert np.array_equal((v * 255).numpy().astype(np.uint8)[0], b)
        y = fvd_mod.preprocess(v)[0]                             # [3,T,224,224]
        assert tuple(y.shape) == (3, b.shape[1], 224, 224)
        flat = y.reshape(-1)
        out["pre_" + tag] = flat[i3d_ref.sample_index(flat.numel(), "pre." + tag, PRE_SAMPLES)].numpy()
    np.savez_compressed(os.path.join(GOLDEN, "i3d_preprocess.npz"), **out)

    # ---- Frechet distance (the reference centres its argument in place: hand it copies)
    out = {}
    for tag, n, d, shift in i3d_ref.FRECHET_CASES:
        f1, f2 = i3d_ref.golden_features(n, d, tag + ".a"), i3d_ref.golden_features(n, d, tag + ".b", shift)
        out["f1_" + tag], out["f2_" + tag] = f1, f2
        out["fd_" + tag] = np.float64(fvd_mod.frechet_distance(torch.from_numpy(f1.copy()), torch.from_numpy(f2.copy())))
        print(f"frechet {tag}: {float(out['fd_' + tag]):.12g}")
    np.savez_compressed(os.path.join(GOLDEN, "i3d_frechet.npz"), **out)
    for name in ("i3d_net", "i3d_preprocess", "i3d_frechet"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
