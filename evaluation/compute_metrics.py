#!/usr/bin/env python3
"""PSNR / SSIM / LPIPS between two folders of videos, on the GPU (the fork's evaluation/compute_metrics.py and, for a --root2 that holds one
sub-folder per experiment, its compute_metrics_threads.py; the kernel needs no thread pool).

Files are paired by name.  `.pt` (torch.load(weights_only=True); [C,T,H,W] or [1,C,T,H,W], values in [-1, 1] as infer.py writes
them) and `.npy` (the same layouts, or uint8 frames [T,H,W,C] as save_videos_grid's fallback writes them) are read directly; `.mp4`
only if imageio is importable - otherwise an .mp4 pair is an error, not a silent skip; `.avi` (Motion-JPEG, what --save-mjpeg writes) is
decoded on the GPU (mjpeg_io.read_mjpeg_clip) to the bytes a player shows and scored like other uint8 frames.  Scores are per frame over the common frames
and averaged over all frames of all pairs; the result file has the reference's lines.  LPIPS (AlexNet, the reference's
compute_lpips) is scored only with --lpips-alexnet PATH [--lpips-linear PATH]: the weights are user-supplied (a torchvision AlexNet
state dict plus the LPIPS linear file, or one full LPIPS state dict), none are shipped or fetched; without them the result file has no
`LPIPS` line.  --fvd-i3d PATH (the I3D state dict i3d_pretrained_400.pt, user-supplied) adds an `FVD:` line when at least two pairs were
scored; with an --fvd-* flag a pair of fewer than ten common frames is an error that stops the run (the reference asserts the same), it is
not skipped: "FVD (videogpt I3D logits)", the fork's calculate_fvd with method='videogpt' - not interchangeable with
the styleganv variant; --motion [--motion-block 8|16] [--motion-radius R] [--motion-lam L] adds `MotionEPE:` and `MotionMean:` lines
(block-matching motion fields of both sides, metrics.motion_compare: this project's own measure, not FVMD); --fvd-synthetic runs it under stand-in weights (not comparable with any published value).  uint8 frames (.npy, .mp4) go through the rescale=False path, so the network sees exactly those bytes."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTS = (".pt", ".npy", ".mp4", ".avi")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Compute PSNR / SSIM (and LPIPS, given weights) between two sets of videos on the GPU.")
    p.add_argument("--root1", type=str, required=True, help="Directory of reference/original videos (.pt, .npy; .mp4 with imageio).")
    p.add_argument("--root2", type=str, required=True, help="Directory of reconstructed videos, or of one sub-folder per experiment.")
    p.add_argument("--results-dir", type=str, required=True, help="Directory to store the metric results.")
    p.add_argument("--lpips-alexnet", type=str, default=None, help="score LPIPS too: a torchvision AlexNet state dict (needs --lpips-linear), "
                                                                   "or one full LPIPS state dict (.pt / .pth / .safetensors; weights are not shipped)")
    p.add_argument("--lpips-linear", type=str, default=None, help="the LPIPS linear layers (lin{0..4}.model.1.weight)")
    from hunyuanvideo_efficiency_amd.metrics import add_fvd_arguments, add_gssim_arguments, add_motion_arguments, motion_from_args
    add_fvd_arguments(p)
    add_gssim_arguments(p)               # --gssim, --metrics-csv PATH
    add_motion_arguments(p)              # --motion [--motion-block B] [--motion-radius R] [--motion-lam L]: MotionEPE / MotionMean lines
    a = p.parse_args(argv)
    a.motion_params = motion_from_args(a, p)
    if a.lpips_linear and not a.lpips_alexnet:
        p.error("--lpips-linear needs --lpips-alexnet")
    if a.fvd_i3d and a.fvd_synthetic:
        p.error("--fvd-synthetic and --fvd-i3d exclude each other")
    return a


def list_videos(root):
    return sorted(f for f in os.listdir(root) if f.endswith(EXTS) and os.path.isfile(os.path.join(root, f)))


def pair_files(root1, root2):
    """names present in both folders, sorted (compute_metrics.py:96-104)"""
    return sorted(set(list_videos(root1)) & set(list_videos(root2)))


def read_video(path):
    """-> (tensor [C,T,H,W] on the host (an .avi: on the GPU), rescale): float videos are in [-1, 1] (rescale=True), uint8 frames become [0, 1] floats"""
    ext = os.path.splitext(path)[1]
    if ext == ".avi":                                   # decoded on the device to byte / 255, the floats of the uint8 branch below
        from hunyuanvideo_efficiency_amd.mjpeg_io import read_mjpeg_clip
        return read_mjpeg_clip(path, "cuda", dtype=torch.float32, unit=True)[0], False
    if ext == ".pt":
        x = torch.load(path, map_location="cpu", weights_only=True)
    elif ext == ".npy":
        x = torch.from_numpy(np.load(path, allow_pickle=False))
    else:
        try:
            import imageio
        except ImportError as e:
            raise RuntimeError(f"{path}: reading .mp4 needs imageio, which is not installed; score the .pt reconstructions instead") from e
        rd = imageio.get_reader(path)
        x = torch.from_numpy(np.stack([np.asarray(f) for f in rd]))
        rd.close()
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{path}: expected one tensor, got {type(x).__name__}")
    if x.dtype == torch.uint8:                          # frames [T,H,W,C] (or [T,H,W]): q / 255 quantises back to q
        if x.dim() == 3:
            x = x[..., None]
        if x.dim() != 4:
            raise ValueError(f"{path}: uint8 frames must be [T,H,W,C], got {tuple(x.shape)}")
        return (x.permute(3, 0, 1, 2).float() / 255.0).contiguous(), False
    if x.dim() == 5 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 4:
        raise ValueError(f"{path}: expected [C,T,H,W] or [1,C,T,H,W], got {tuple(x.shape)}")
    return x, True


def score_folders(root1, root2, results_dir, device="cuda", lpips=None, fvd=None, gssim=False, metrics_csv=None, motion=None):
    """`motion` ({"block", "radius", "lam"}, --motion): every pair's block-matching motion fields are compared too and the result file gains
    `MotionEPE:` and `MotionMean:` lines (metrics.motion_compare; this project's own measure, not FVMD - the csv's `fvdm` stays blank)"""
    from hunyuanvideo_efficiency_amd.metrics import MetricsAccumulator, motion_compare
    names = pair_files(root1, root2)
    if not names:
        print(f"No matching video files between {root1} and {root2}.")
        return None
    print(f"Found {len(names)} matching pairs.")
    acc = MetricsAccumulator(lpips=lpips, fvd=fvd, gssim=gssim, csv=metrics_csv is not None)
    for name in names:
        v1, r1 = read_video(os.path.join(root1, name))
        v2, r2 = read_video(os.path.join(root2, name))
        if r1 != r2:
            raise ValueError(f"{name}: one side holds uint8 frames and the other float video")
        dt = torch.float16 if v1.dtype == torch.float16 and v2.dtype == torch.float16 else torch.float32
        m = acc.add_video(v1.to(device, dtype=dt), v2.to(device, dtype=dt), rescale=r1,
                          names=[os.path.abspath(os.path.join(root2, name))] if acc.csv else None)
        if motion is not None:
            acc.add_motion(motion_compare(v1.to(device, dtype=dt), v2.to(device, dtype=dt), rescale=r1, **motion))
        print(f"{name}: PSNR {m['psnr_mean']:.4f} SSIM {m['ssim_mean']:.6f}" + (f" LPIPS {m['lpips_mean']:.6f}" if lpips is not None else "")
              + (f" SSIM3D {m['ssim3d']:.6f} SSIM2D {m['ssim2d']:.6f}" if gssim else "") + f" ({len(m['psnr'])} frames)")
    results = acc.result()
    path = acc.save(results_dir, root1, root2)
    print(f"Results: {results}{acc.fvd_note()}\nSaved to {path}")
    if metrics_csv is not None:
        print(f"Saved per-clip rows to {acc.save_csv(metrics_csv)}")
    return path


def main(argv=None):
    a = parse_args(argv)
    lpips = None
    if a.lpips_alexnet:
        from hunyuanvideo_efficiency_amd.metrics import LpipsAlex
        lpips = LpipsAlex.from_files(a.lpips_alexnet, a.lpips_linear)
    from hunyuanvideo_efficiency_amd.metrics import fvd_from_args
    fvd = fvd_from_args(a)
    subdirs = sorted(d for d in os.listdir(a.root2) if os.path.isdir(os.path.join(a.root2, d)))
    if subdirs and not list_videos(a.root2):            # one folder per experiment: one result file each
        csv_of = lambda d: None if a.metrics_csv is None else "{0}_{2}{1}".format(*os.path.splitext(a.metrics_csv), d)   # noqa: E731
        return [score_folders(a.root1, os.path.join(a.root2, d), os.path.join(a.results_dir, d), lpips=lpips, fvd=fvd, gssim=a.gssim,
                              metrics_csv=csv_of(d), motion=a.motion_params) for d in subdirs]
    return [score_folders(a.root1, a.root2, a.results_dir, lpips=lpips, fvd=fvd, gssim=a.gssim, metrics_csv=a.metrics_csv,
                          motion=a.motion_params)]


if __name__ == "__main__":
    main()
