#!/usr/bin/env python3
"""VAE reconstruction driver of the fork (infer.py:1-127) on the MI355X kernels: for every `<name>.pt` video tensor [C,T,H,W] in
--tensor-dir, run AutoencoderKLCausal3D.forward (encode -> posterior.mode() -> decode) under the temporal-op configuration of
--config-json (t_ops_config.json) and write the reconstruction to --output-dir/<name>.pt.  Same flags as the reference; input
tensors and checkpoints are read with torch.load(weights_only=True) only.  With --yuv-format {I420,NV12,YV12} --tensor-dir is a folder
of raw planar YUV 4:2:0 files instead, converted to clips on the GPU (hunyuanvideo_efficiency_amd/dataset.py; --target-height,
--start-frame, --end-frame as dataset_processor/yuv_tensor.py takes them); outputs keep the input file's stem.  With --save-yuv
{y4m,I420,YV12,NV12} every reconstruction is also written as 8-bit YUV 4:2:0, converted on the GPU
(hunyuanvideo_efficiency_amd/video_io.py), under a name that --yuv-format reads back; with --save-mjpeg [--save-quality Q]
[--save-strip N] as <name>.avi, Motion-JPEG coded on the GPU (hunyuanvideo_efficiency_amd/mjpeg_io.py; lossy), and <name>_strip.jpg, N evenly spaced frames side by side; with --mjpeg-input
[--start-frame A] [--end-frame B] --tensor-dir is a folder of such .avi files, decoded on the GPU.  Without --vae-path
the VAE gets deterministic synthetic weights (there are no checkpoints in this environment): the plumbing and the kernels are what is
exercised.  With --score --motion [--motion-block 8|16] [--motion-radius R] [--motion-lam L] every clip also gets <name>_motion.json:
block-matching motion of input and reconstruction (metrics.motion_compare; this project's own measure, not FVMD)."""
import argparse
import json
import os

import torch


class VideoTensorDataset:
    """dataset_processor/dataset_loader.py:9-24: sorted *.pt files, each a (C, T, H, W) tensor; returns (tensor, file name)."""

    def __init__(self, tensor_dir):
        self.tensor_dir = tensor_dir
        self.tensor_files = sorted(f for f in os.listdir(tensor_dir) if f.endswith(".pt"))

    def __len__(self):
        return len(self.tensor_files)

    def __getitem__(self, idx):
        path = os.path.join(self.tensor_dir, self.tensor_files[idx])
        return torch.load(path, map_location="cpu", weights_only=True), self.tensor_files[idx]


def infer_vae(model, dataset, device, output_dir, max_files=None, batch_size=1, scorer=None, save=True, spectrum_dir=None, fps=None,
              content_dir=None, save_yuv=None, motion_dir=None, motion=None, mjpeg=None):
    """Reconstructs the first `max_files` tensors, `batch_size` at a time (tensors of one batch must have equal shapes, as a
    DataLoader's default collate requires); every input still gets its own <name>.pt of shape [1, C, T, H, W].
    `scorer` (a metrics.MetricsAccumulator): each reconstruction is scored against its input while both are on the device
    (PSNR / SSIM, and LPIPS if the accumulator holds LPIPS weights, per frame of the common frames; with I3D weights the accumulator also
    keeps both clips' logits for the FVD of the whole run).  save=False skips the copy to the host and the .pt files.
    `spectrum_dir`: also write <name>_spectrum.json there per input - the temporal spectra (metrics.spectrum_report; the fork's
    theory_analysis.ipynb) of the input, of the posterior mean the forward already returns and of the reconstruction, with `freq` axes
    when `fps` is given.  `content_dir`: also write <name>_content.json there per input - {"input", "reconstruction"}, each the dict
    of metrics.content_entropy (inter- / intra-frame entropy of the 8-bit gray frames, this project's definition): comparing the two
    `inter_entropy` values shows how much frame-to-frame detail the configuration removed.
    `save_yuv` ("y4m" | "I420" | "YV12" | "NV12"): every reconstruction is also written as 8-bit YUV 4:2:0, converted on the device
    (video_io.save_reconstruction), whatever `save` says: <name>.y4m or <name>_<n>fps_<w>x<h>.yuv, at the input file's rate, else `fps`,
    else 24; their paths are returned too.
    `mjpeg` ({"quality", "strip"}): every reconstruction is also written as <name>.avi (mjpeg_io.save_reconstruction_mjpeg), and as
    <name>_strip.jpg when "strip" is a frame count, at the same rate, whatever `save` says; their paths are returned too.
    `motion_dir` with `motion` ({"block", "radius", "lam"}): also write <name>_motion.json there per input - the dict of
    metrics.motion_compare (block-matching motion of input and reconstruction, the end-point error between the two fields; this project's
    own measure, not FVMD)."""
    if batch_size < 1:
        raise ValueError(f"--batch-size must be >= 1, got {batch_size}")
    os.makedirs(output_dir, exist_ok=True)
    from hunyuanvideo_efficiency_amd.dataset import clip_stem
    if spectrum_dir is not None:
        from hunyuanvideo_efficiency_amd.metrics import spectrum_json, spectrum_report
        os.makedirs(spectrum_dir, exist_ok=True)
    if content_dir is not None:
        from hunyuanvideo_efficiency_amd.metrics import content_entropy_many
        os.makedirs(content_dir, exist_ok=True)
    if motion_dir is not None:
        from hunyuanvideo_efficiency_amd.metrics import motion_compare
        os.makedirs(motion_dir, exist_ok=True)
    file_fps = getattr(dataset, "fps", {})       # a YuvClipDataset knows each file's frame rate from its name
    n = len(dataset) if max_files is None else min(len(dataset), max_files)
    done = []
    for start in range(0, n, batch_size):
        items = [dataset[idx] for idx in range(start, min(n, start + batch_size))]
        shapes = {tuple(v.shape) for v, _ in items}
        if len(shapes) != 1:
            raise ValueError(f"a batch needs tensors of one shape, got {sorted(shapes)} for {[f for _, f in items]}")
        names = [clip_stem(f) for _, f in items]
        video = torch.stack([v for v, _ in items]).to(device, dtype=torch.float16)      # the DataLoader's batch dimension
        print(f"Processing {', '.join(names)}, video shape: {tuple(video.shape)}")
        with torch.no_grad():
            fwd = model(video, return_dict=False, return_posterior=True, sample_posterior=False)
        recon = fwd[0]
        if spectrum_dir is not None:
            posterior = fwd[1]
            for b, name in enumerate(names):
                rep = spectrum_report(video[b], posterior.mean[b], recon[b], fps=fps if fps is not None else file_fps.get(items[b][1]))
                with open(os.path.join(spectrum_dir, f"{name}_spectrum.json"), "w") as f:
                    json.dump(spectrum_json(rep), f)
                print(f"Spectrum {name}: high-band share input {rep['input']['high_band_share']:.4f} latent "
                      f"{rep['latent']['high_band_share']:.4f} reconstruction {rep['reconstruction']['high_band_share']:.4f} "
                      f"(cutoff bin {rep['input']['cutoff_bin']} of {video.shape[2]} frames)")
        if content_dir is not None:
            stats = content_entropy_many([video[b] for b in range(len(names))] + [recon[b] for b in range(len(names))])
            for b, name in enumerate(names):
                c = {"input": stats[b], "reconstruction": stats[len(names) + b]}
                with open(os.path.join(content_dir, f"{name}_content.json"), "w") as f:
                    json.dump(c, f)
                fmt = lambda v: "n/a" if v is None else f"{v:.4f}"      # noqa: E731  (a single frame has no inter-frame entropy)
                print(f"Content {name}: inter-frame entropy input {fmt(c['input']['inter_entropy'])} reconstruction "
                      f"{fmt(c['reconstruction']['inter_entropy'])} bits, intra-frame {fmt(c['input']['intra_entropy'])} / "
                      f"{fmt(c['reconstruction']['intra_entropy'])} (this project's definition)")
        if motion_dir is not None:
            fmt = lambda v: "n/a" if v is None else f"{v:.4f}"          # noqa: E731  (a single frame has no motion)
            for b, name in enumerate(names):
                c = motion_compare(video[b], recon[b], **motion)
                with open(os.path.join(motion_dir, f"{name}_motion.json"), "w") as f:
                    json.dump(c, f)
                print(f"Motion {name}: input {fmt(c['ref']['motion_mean'])} reconstruction {fmt(c['rec']['motion_mean'])} px/frame, "
                      f"end-point error {fmt(c['motion_epe'])} px (block {motion['block']}, radius {motion['radius']}; this project's own "
                      "measure, not FVMD)")
        if scorer is not None:
            m = scorer.add_video(video, recon, rescale=True,
                                 names=[os.path.abspath(os.path.join(output_dir, f"{name}.pt")) for name in names] if scorer.csv else None)
            for b, name in enumerate(names):
                lp = f" LPIPS {m['lpips'][b].mean():.6f}" if "lpips" in m else ""
                if scorer.gssim:
                    lp += f" SSIM3D {m['ssim3d'][b]:.6f} SSIM2D {m['ssim2d'][b]:.6f}"
                print(f"Scored {name}: PSNR {m['psnr'][b].mean():.4f} SSIM {m['ssim'][b].mean():.6f}{lp} ({m['psnr'].shape[1]} frames)")
        if save_yuv is not None:
            from hunyuanvideo_efficiency_amd.video_io import save_reconstruction
            for b, name in enumerate(names):
                rate = file_fps.get(items[b][1], fps)
                done.append(save_reconstruction(recon[b], output_dir, name, save_yuv, rate))
                print(f"Saved reconstructed video to {done[-1]}, {recon.shape[2]} frames of {recon.shape[4]} x {recon.shape[3]}")
        if mjpeg is not None:
            from hunyuanvideo_efficiency_amd.mjpeg_io import save_reconstruction_mjpeg
            for b, name in enumerate(names):
                for path in save_reconstruction_mjpeg(recon[b], output_dir, name, file_fps.get(items[b][1], fps), mjpeg["quality"], mjpeg["strip"]):
                    done.append(path)
                    print(f"Saved reconstructed video to {path}, {recon.shape[2]} frames of {recon.shape[4]} x {recon.shape[3]}")
        if not save:
            continue
        recon = recon.cpu().float()
        for b, name in enumerate(names):
            out_path = os.path.join(output_dir, f"{name}.pt")
            torch.save(recon[b:b + 1].clone(), out_path)
            print(f"Saved reconstructed video to {out_path}, shape: {tuple(recon[b:b + 1].shape)}")
            done.append(out_path)
    return done


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="VAE inference script for video tensors (MI355X kernels).")
    p.add_argument("--tensor-dir", type=str, required=True, help="Directory containing input .pt video tensors.")
    p.add_argument("--output-dir", type=str, required=True, help="Directory to save the reconstructed videos.")
    p.add_argument("--vae-path", type=str, default=None, help="VAE checkpoint directory (config.json + pytorch_model.pt); "
                                                            "default: synthetic weights")
    p.add_argument("--config-json", type=str, default=None, help="Path to the T-ops config JSON file (t_ops_config.json).")
    p.add_argument("--max-files", type=int, default=None)
    p.add_argument("--mp4", action="store_true", help="accepted for flag compatibility; mp4 writing is outside this build (SURVEY 8f row 4)")
    p.add_argument("--batch-size", type=int, default=1, help="videos per forward (equal shapes); the VAE runs them one after another")
    p.add_argument("--num-workers", type=int, default=4)
    p.add_argument("--reduced", action="store_true", help="synthetic-weight mode only: reduced channel widths (32,64,128,128)")
    p.add_argument("--score", action="store_true", help="score every reconstruction against its input on the GPU (PSNR / SSIM per frame, "
                                                       "evaluation/compute_metrics.py without the mp4 round trip) and write metrics_<timestamp>.txt")
    p.add_argument("--results-dir", type=str, default=None, help="with --score: where the result file goes (default: --output-dir)")
    p.add_argument("--no-save", action="store_true", help="with --score: do not copy reconstructions to the host or write .pt files")
    p.add_argument("--lpips-alexnet", type=str, default=None, help="with --score: score LPIPS too - a torchvision AlexNet state dict (needs "
                                                                   "--lpips-linear) or one full LPIPS state dict; weights are not shipped")
    p.add_argument("--lpips-linear", type=str, default=None, help="with --lpips-alexnet: the LPIPS linear layers (lin{0..4}.model.1.weight)")
    p.add_argument("--lpips-synthetic", action="store_true", help="with --score: LPIPS under deterministic synthetic weights (exercises the "
                                                                  "kernels; NOT comparable with published LPIPS)")
    from hunyuanvideo_efficiency_amd.metrics import add_fvd_arguments
    add_fvd_arguments(p)                 # --fvd-i3d PATH | --fvd-synthetic, with --score
    p.add_argument("--spectrum", action="store_true", help="with --score: write <name>_spectrum.json per clip into the results directory - "
                                                          "temporal spectra of input, latent and reconstruction and their high-band shares")
    p.add_argument("--fps", type=float, default=None, help="with --spectrum: frame rate of the clips, adds the frequency axes; with "
                                                           "--save-yuv / --save-mjpeg: the rate written (default with --yuv-format: the rate in each "
                                                           "file's name)")
    p.add_argument("--content", action="store_true", help="with --score: write <name>_content.json per clip into the results directory - "
                                                         "inter- / intra-frame entropy of input and reconstruction (this project's definition)")
    from hunyuanvideo_efficiency_amd.metrics import add_gssim_arguments, add_motion_arguments, motion_from_args
    add_motion_arguments(p)              # --motion [--motion-block B] [--motion-radius R] [--motion-lam L], with --score
    add_gssim_arguments(p)               # --gssim, --metrics-csv PATH, with --score
    from hunyuanvideo_efficiency_amd.dataset import add_yuv_arguments, check_yuv_arguments
    add_yuv_arguments(p)                 # --yuv-format {I420,NV12,YV12} [--target-height N] [--start-frame A] [--end-frame B]
    from hunyuanvideo_efficiency_amd.video_io import add_save_yuv_argument
    add_save_yuv_argument(p)             # --save-yuv {y4m,I420,YV12,NV12}
    from hunyuanvideo_efficiency_amd.mjpeg_io import add_save_mjpeg_arguments, check_save_mjpeg_arguments
    add_save_mjpeg_arguments(p)          # --save-mjpeg [--save-quality Q] [--save-strip N]
    from hunyuanvideo_efficiency_amd.mjpeg_io import add_mjpeg_input_arguments
    add_mjpeg_input_arguments(p)         # --mjpeg-input [--start-frame A] [--end-frame B]: --tensor-dir holds .avi files
    a = p.parse_args(argv)
    check_yuv_arguments(a, p)
    quality = check_save_mjpeg_arguments(p, a)
    a.mjpeg_params = dict(quality=quality, strip=a.save_strip) if a.save_mjpeg else None
    if a.spectrum and not a.score:
        p.error("--spectrum is only valid with --score")
    if a.content and not a.score:
        p.error("--content is only valid with --score")
    a.motion_params = motion_from_args(a, p)
    if a.motion and not a.score:
        p.error("--motion is only valid with --score")
    if (a.gssim or a.metrics_csv) and not a.score:
        p.error("--gssim and --metrics-csv are only valid with --score")
    if a.fps is not None and not (a.spectrum or a.save_yuv or a.save_mjpeg):
        p.error("--fps is only valid with --spectrum, --save-yuv or --save-mjpeg")
    if a.fps is not None and not a.fps > 0:
        p.error("--fps must be positive")
    if (a.lpips_alexnet or a.lpips_linear or a.lpips_synthetic) and not a.score:
        p.error("--lpips-* flags are only valid with --score")
    if a.lpips_linear and not a.lpips_alexnet:
        p.error("--lpips-linear needs --lpips-alexnet")
    if a.lpips_synthetic and a.lpips_alexnet:
        p.error("--lpips-synthetic and --lpips-alexnet exclude each other")
    if (a.fvd_i3d or a.fvd_synthetic) and not a.score:
        p.error("--fvd-* flags are only valid with --score")
    if a.fvd_i3d and a.fvd_synthetic:
        p.error("--fvd-synthetic and --fvd-i3d exclude each other")
    if a.no_save and not (a.score or a.save_yuv or a.save_mjpeg):
        p.error("--no-save is only valid with --score, --save-yuv or --save-mjpeg (nothing would be produced)")
    if a.results_dir and not a.score:
        p.error("--results-dir is only valid with --score")
    return a


def main(argv=None):
    a = parse_args(argv)
    device = "cuda"
    from hunyuanvideo_efficiency_amd import synthetic as syn
    from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D, load_vae
    if a.vae_path:
        vae = load_vae("884-16c-hy", "fp16", vae_path=a.vae_path, device=device, t_ops_config_path=a.config_json, test=True,
                       with_encoder=True)[0]
    else:
        boc = (32, 64, 128, 128) if a.reduced else syn.VAE_BLOCK_OUT_CHANNELS
        vae = AutoencoderKLCausal3D(block_out_channels=boc, device=device, with_encoder=True)
        vae.load_state_dict({k: v.to(torch.float16) for k, v in syn.synth_vae_state_dict(boc, seed=0, encoder=True).items()}, strict=True)
        if a.config_json:
            from hunyuanvideo_efficiency_amd.vae import _apply_t_ops_config_to_vae, load_t_ops_config
            _apply_t_ops_config_to_vae(vae, load_t_ops_config(a.config_json))
    if a.yuv_format or a.mjpeg_input:
        from hunyuanvideo_efficiency_amd.dataset import dataset_from_args
        dataset = dataset_from_args(a, device)
    else:
        dataset = VideoTensorDataset(a.tensor_dir)
    if not a.score:
        return infer_vae(vae, dataset, device, a.output_dir, a.max_files, a.batch_size, save=not a.no_save, fps=a.fps, save_yuv=a.save_yuv,
                         mjpeg=a.mjpeg_params)
    from hunyuanvideo_efficiency_amd.metrics import MetricsAccumulator, fvd_from_args, lpips_from_args
    scorer = MetricsAccumulator(lpips=lpips_from_args(a), fvd=fvd_from_args(a, score=a.score), gssim=a.gssim, csv=bool(a.metrics_csv))
    done = infer_vae(vae, dataset, device, a.output_dir, a.max_files, a.batch_size, scorer, not a.no_save,
                     (a.results_dir or a.output_dir) if a.spectrum else None, a.fps, (a.results_dir or a.output_dir) if a.content else None,
                     a.save_yuv, (a.results_dir or a.output_dir) if a.motion_params else None, a.motion_params, a.mjpeg_params)
    results = scorer.result()
    print(f"Results over {scorer.frames} frames: {results}" + (" (LPIPS under synthetic weights: not comparable with published LPIPS)"
                                                               if a.lpips_synthetic else "") + scorer.fvd_note())
    path = scorer.save(a.results_dir or a.output_dir, a.tensor_dir, a.output_dir)
    print(f"Saved metrics to {path}")
    if a.metrics_csv:
        print(f"Saved per-clip rows to {scorer.save_csv(a.metrics_csv)}")
    return done


if __name__ == "__main__":
    main()
