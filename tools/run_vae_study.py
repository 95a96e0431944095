#!/usr/bin/env python3
"""The VAE efficiency study in one process: enumerate temporal-op configurations (dynamic_enumeration.py), and for each one build
the VAE under it, reconstruct every video of --tensor-dir and score it on the GPU (PSNR / SSIM per frame, nothing copied to the host
or written per video: infer.py --score --no-save).  One line per configuration is appended to <output-dir>/study.jsonl:
{"config", "PSNR", "SSIM", ("LPIPS" with --lpips-alexnet / --lpips-synthetic,) "frames", "compression": T_latent / T_in, ("spectrum" with
--spectrum: the high-band shares of input, latent and reconstruction averaged over clips; the mean spectra go to spectra_<config>.json)} - or {"config", "refused": message} for a configuration the
VAE refuses (a ValueError of its list-length checks, NotImplementedError).  Configurations run one after another on one GPU: the
fork's shell drivers' background batches over several cards are not reproduced.

  python tools/run_vae_study.py --tensor-dir D --output-dir O [--base-config t_ops_config.json] [--mode pool] [--limit N] [--reduced]
  python tools/run_vae_study.py --tensor-dir D --output-dir O --config-dir DIR_OF_JSONS
  ... --lpips-alexnet ALEXNET.pth --lpips-linear ALEX_LIN.pth   (user-supplied weights; --lpips-synthetic: stand-in weights, the
                                                                 record then carries "lpips_weights": "synthetic")
  ... --fvd-i3d i3d_pretrained_400.pt   (user-supplied; --fvd-synthetic: stand-in weights) adds "fvd", "fvd_clips", "fvd_variant": FVD
                                        (videogpt I3D logits) of the inputs against each configuration's reconstructions - not the
                                        styleganv variant; the inputs' logits are computed once for all configurations
  ... --yuv-format I420 [--target-height 240] [--start-frame A] [--end-frame B]   --tensor-dir is a folder of raw planar YUV 4:2:0 files
                                        (<name>_<n>fps_<w>x<h>.yuv), converted on the GPU once for all configurations and kept on the
                                        device; with --spectrum and no --fps each file name's frame rate gives the frequency axes
  ... --gssim                           each record gains "ssim3d" and "ssim2d": the Gaussian-window SSIMs of the fork's rebuttal tables
                                        (run.py's pytorch_msssim call, whose window spans frames, and calculate_ssim.py's per-frame one)
  ... --motion [--motion-block 8|16] [--motion-radius R] [--motion-lam L]
                                        each record gains "motion": block-matching motion of inputs and reconstructions and the end-point
                                        error between their fields (metrics.motion_summary; this project's own measure, not FVMD)
  ... --content                         each record gains "content": inter- / intra-frame entropy, mean |difference| and TI of the inputs
                                        and of the reconstructions (metrics.content_entropy, this project's definition) and
                                        "inter_entropy_drop", the frame-to-frame detail the configuration removed; the inputs' values
                                        are computed once for all configurations
  ... --bucket-dir B                    the fork's run_experiments_buckets.sh: the sweep runs once per <bucket>.txt list of folder B
                                        (tools/bucket_clips.py writes them), on the clips of --tensor-dir whose file stems the list
                                        names; records go to <output-dir>/<bucket>/study.jsonl and carry "bucket".  A list that names a
                                        clip absent from --tensor-dir is an error
  ... --interp-mode trilinear           with --base-config: every decoder block of each enumerated configuration gets this
                                        "interp_mode" (nearest | nearest-exact | area | trilinear) before it is written; without the
                                        flag the configurations are written as enumerated"""
import argparse
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_vae(config_json, vae_path, reduced, device):
    from hunyuanvideo_efficiency_amd import synthetic as syn
    from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D, _apply_t_ops_config_to_vae, load_t_ops_config, load_vae
    if vae_path:
        return load_vae("884-16c-hy", "fp16", vae_path=vae_path, device=device, t_ops_config_path=config_json, test=True, with_encoder=True)[0]
    boc = (32, 64, 128, 128) if reduced else syn.VAE_BLOCK_OUT_CHANNELS
    vae = AutoencoderKLCausal3D(block_out_channels=boc, device=device, with_encoder=True)
    vae.load_state_dict({k: v.to(torch.float16) for k, v in syn.synth_vae_state_dict(boc, seed=0, encoder=True).items()}, strict=True)
    _apply_t_ops_config_to_vae(vae, load_t_ops_config(config_json))
    return vae


def run_config(config_json, dataset, vae_path, reduced, device, max_files=None, lpips=None, spectra=None, fps=None, fvd=None,
               input_logits=None, input_content=None, gssim=False, save_yuv=None, save_dir=None, motion=None, input_motion=None,
               mjpeg=None):
    """-> the study.jsonl record of one configuration.  `fvd` (an I3D, --fvd-i3d / --fvd-synthetic): the record gains "fvd" - FVD
    (videogpt I3D logits) between the inputs and this configuration's reconstructions, None below two clips - and "fvd_clips";
    `input_logits` (a dict the caller keeps across configurations) holds every input clip's logits, which do not depend on the
    configuration: they are computed once.  `spectra` (a dict, --spectrum): temporal spectra are taken too - the record gains
    "spectrum" and the dict is filled with the configuration's mean spectra (`mean_spectra`).  `input_content` (a dict the caller keeps
    across configurations, --content): the record gains "content" (metrics.content_summary); the dict holds every input clip's
    statistics, computed once.  `gssim` (--gssim): the record gains "ssim3d" and "ssim2d", the Gaussian-window SSIMs of the fork's rebuttal
    tables (metrics.gaussian_ssim), each the mean over the clips.  `save_yuv` (--save-yuv) with `save_dir`: every reconstruction is written
    there as 8-bit YUV 4:2:0, converted on the device (video_io.save_reconstruction); the record gains "saved", the folder.  `motion`
    ({"block", "radius", "lam"}, --motion) with `input_motion` (a dict the caller keeps across configurations): the record gains "motion"
    (metrics.motion_summary: block-matching motion of inputs and reconstructions and the end-point error between their fields, this
    project's own measure, not FVMD); the dict holds every input clip's field, computed once.  `mjpeg` ({"quality", "strip"},
    --save-mjpeg) with `save_dir`: every reconstruction is written there as <name>.avi, Motion-JPEG coded on the device
    (mjpeg_io.save_reconstruction_mjpeg), and as <name>_strip.jpg when "strip" is a frame count; the record gains "saved" as well"""
    from hunyuanvideo_efficiency_amd.metrics import MetricsAccumulator
    rec = {"config": os.path.basename(config_json)}
    try:
        vae = build_vae(config_json, vae_path, reduced, device)
        acc = MetricsAccumulator(lpips=lpips, fvd=fvd, gssim=gssim)
        input_logits = {} if input_logits is None else input_logits
        t_in = t_lat = 0
        reports = []
        content_jobs = []                               # (clip index or None for a reconstruction, enqueued job): one synchronisation below
        motion_jobs = []                                # the same for the motion fields
        n = len(dataset) if max_files is None else min(len(dataset), max_files)
        for idx in range(n):
            video, file_name = dataset[idx]
            video = video[None].to(device, dtype=torch.float16)
            clip_fps = fps if fps is not None else getattr(dataset, "fps", {}).get(file_name)   # raw YUV files carry their rate
            with torch.no_grad():
                z = vae.encode(video).latent_dist.mode()
                recon = vae.decode(z).sample
            m = acc.add_video(video, recon, rescale=True, ref_logits=input_logits.get((idx, min(video.shape[2], recon.shape[2]))))
            if fvd is not None:                         # keyed by the frames scored: a configuration may shorten the clip
                input_logits[(idx, min(video.shape[2], recon.shape[2]))] = m["fvd_ref_logits"]
            if spectra is not None:
                from hunyuanvideo_efficiency_amd.metrics import spectrum_report
                reports.append(spectrum_report(video[0], z[0], recon[0], fps=clip_fps))
            if input_content is not None:
                from hunyuanvideo_efficiency_amd import metrics
                if idx not in input_content:
                    content_jobs.append((idx, metrics._content_enqueue(video[0])))
                content_jobs.append((None, metrics._content_enqueue(recon[0])))
            if motion is not None:
                from hunyuanvideo_efficiency_amd import metrics
                if idx not in input_motion:
                    motion_jobs.append((idx, metrics._motion_enqueue(video[0], **motion)))
                motion_jobs.append((None, metrics._motion_enqueue(recon[0], **motion)))
            if save_yuv is not None:
                from hunyuanvideo_efficiency_amd.dataset import clip_stem
                from hunyuanvideo_efficiency_amd.video_io import save_reconstruction
                # the input file's rate first, as infer.py does
                save_reconstruction(recon[0], save_dir, clip_stem(file_name), save_yuv, getattr(dataset, "fps", {}).get(file_name, fps))
                rec["saved"] = save_dir
            if mjpeg is not None:         # --save-mjpeg: <name>.avi (and <name>_strip.jpg) in the same folder, at the same rate
                from hunyuanvideo_efficiency_amd.dataset import clip_stem
                from hunyuanvideo_efficiency_amd.mjpeg_io import save_reconstruction_mjpeg
                save_reconstruction_mjpeg(recon[0], save_dir, clip_stem(file_name), getattr(dataset, "fps", {}).get(file_name, fps),
                                          mjpeg["quality"], mjpeg["strip"])
                rec["saved"] = save_dir
            t_in += video.shape[2]
            t_lat += z.shape[2]
        res = acc.result()
        if fvd is not None:
            rec["fvd"] = res.pop("FVD", None)
            rec["fvd_clips"] = acc.clips
            rec["fvd_variant"] = "videogpt I3D logits" + (", synthetic weights" if fvd.label == "synthetic" else "")
        if gssim:
            rec_gssim = {"ssim3d": res.pop("SSIM3D", None), "ssim2d": res.pop("SSIM2D", None)}
        rec.update(res)
        if gssim:
            rec.update(rec_gssim)
        if lpips is not None and lpips.label == "synthetic":
            rec["lpips_weights"] = "synthetic"          # not comparable with published LPIPS
        rec["frames"] = acc.frames
        rec["compression"] = t_lat / t_in if t_in else None
        if input_content is not None:
            from hunyuanvideo_efficiency_amd import metrics
            stats = metrics._content_to_host([j for _, j in content_jobs]) if content_jobs else []
            input_content.update({i: d for (i, _), d in zip(content_jobs, stats) if i is not None})
            rec["content"] = metrics.content_summary([input_content[i] for i in range(n)], [d for (i, _), d in zip(content_jobs, stats) if i is None])
        if motion is not None:
            from hunyuanvideo_efficiency_amd import metrics
            fields = metrics._motion_to_host([j for _, j in motion_jobs]) if motion_jobs else []
            input_motion.update({i: f for (i, _), f in zip(motion_jobs, fields) if i is not None})
            recs = [f for (i, _), f in zip(motion_jobs, fields) if i is None]
            rec["motion"] = metrics.motion_summary([metrics.motion_field_stats(input_motion[i]) for i in range(n)],
                                                   [metrics.motion_compare_fields(input_motion[i], recs[i]) for i in range(n)])
        if spectra is not None:
            rec["spectrum"] = {f"{name}_high_band_share": (sum(r[name]["high_band_share"] for r in reports) / len(reports) if reports else None)
                               for name in ("input", "latent", "reconstruction")}
            spectra.update(mean_spectra(reports))
    except (ValueError, NotImplementedError) as e:
        rec["refused"] = f"{type(e).__name__}: {e}"
    return rec


def mean_spectra(reports):
    """per part (input / latent / reconstruction) the spectra averaged over the clips of one frame count (clips of different lengths have
    different bins: one entry per length), as plain lists: the spectra_<config>.json of --spectrum"""
    import numpy as np
    out = {}
    for name in ("input", "latent", "reconstruction"):
        by_len = {}
        for r in reports:
            by_len.setdefault(len(r[name]["power"]), []).append(r[name])
        out[name] = []
        for T, rs in sorted(by_len.items()):
            e = {"frames": T, "clips": len(rs), "cutoff_bin": rs[0]["cutoff_bin"],
                 "magnitude": np.mean([r["magnitude"] for r in rs], axis=0).tolist(),
                 "power": np.mean([r["power"] for r in rs], axis=0).tolist(),
                 "high_band_share": float(np.mean([r["high_band_share"] for r in rs]))}
            if "freq" in rs[0]:
                e["freq"] = rs[0]["freq"].tolist()
            out[name].append(e)
    return out


class ConvertedOnce:
    """A YuvClipDataset whose clips are converted on first use and then kept on the device (fp16 [3,T,H,W] each): every configuration
    of the study reads the same inputs, so a file is read, uploaded and converted once, not once per configuration."""

    def __init__(self, dataset):
        self.dataset, self.fps, self._items = dataset, dataset.fps, {}
        self.tensor_files = dataset.tensor_files

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, idx):
        if idx not in self._items:
            self._items[idx] = self.dataset[idx]
        return self._items[idx]


class ClipSubset:
    """the clips `indices` of a dataset, under the dataset's surface (len, [i] -> (clip, file name), tensor_files, fps)"""

    def __init__(self, dataset, indices):
        self.dataset, self.indices = dataset, list(indices)
        self.tensor_files = [dataset.tensor_files[i] for i in self.indices]
        if hasattr(dataset, "fps"):
            self.fps = dataset.fps

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, idx):
        return self.dataset[self.indices[idx]]


def read_bucket_lists(bucket_dir, tensor_files):
    """The <bucket>.txt lists of `bucket_dir`, sorted by name -> [(bucket, [index into tensor_files, ...])].  A line names a clip by path
    or file name; it is matched by file stem (the fork's script maps x.mp4 to x.pt).  ValueError for a folder without lists, an empty
    list, and a list that names a clip `tensor_files` does not hold: such a clip is not skipped."""
    from hunyuanvideo_efficiency_amd.dataset import clip_stem
    by_stem = {clip_stem(f): i for i, f in enumerate(tensor_files)}
    names = sorted(f for f in os.listdir(bucket_dir) if f.endswith(".txt"))
    if not names:
        raise ValueError(f"--bucket-dir {bucket_dir} holds no <bucket>.txt list")
    out = []
    for name in names:
        with open(os.path.join(bucket_dir, name)) as f:
            lines = [ln.strip() for ln in f if ln.strip()]
        if not lines:
            raise ValueError(f"bucket list {name} is empty")
        idx = []
        for ln in lines:
            stem = os.path.splitext(os.path.basename(ln))[0]
            if stem not in by_stem:
                raise ValueError(f"bucket list {name} names {ln!r}, but the tensor folder has no clip with the stem {stem!r}")
            if by_stem[stem] not in idx:
                idx.append(by_stem[stem])
        out.append((name[:-len(".txt")], idx))
    return out


INTERP_MODES = ("nearest", "nearest-exact", "area", "trilinear")       # the modes AutoencoderKLCausal3D has kernels for


def override_interp_mode(paths, mode):
    """--interp-mode: rewrite the configuration files `paths` with `interp_mode` = mode in every decoder block"""
    for path in paths:
        with open(path) as f:
            cfg = json.load(f)
        for bc in cfg.get("decoder", {}).get("up_blocks", []):
            bc["interp_mode"] = mode
        with open(path, "w") as f:
            json.dump(cfg, f, indent=2)


def _exp_order(name):
    m = re.search(r"(\d+)", name)
    return (int(m.group(1)) if m else 0, name)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="VAE temporal-op study: enumerate, reconstruct and score on one GPU.")
    p.add_argument("--tensor-dir", required=True, help="input .pt video tensors [C,T,H,W]")
    p.add_argument("--output-dir", required=True, help="study.jsonl and the enumerated configurations go here")
    p.add_argument("--base-config", default=None, help="t_ops_config.json to enumerate from")
    p.add_argument("--config-dir", default=None, help="use the exp_<n>.json files of this folder instead of enumerating")
    p.add_argument("--mode", choices=("pool", "stride", "stride2"), default="pool")
    p.add_argument("--limit", type=int, default=None, help="only the first N configurations")
    p.add_argument("--max-files", type=int, default=None)
    p.add_argument("--vae-path", default=None, help="VAE checkpoint directory; default: synthetic weights")
    p.add_argument("--reduced", action="store_true", help="synthetic-weight mode only: reduced channel widths")
    p.add_argument("--spectrum", action="store_true", help="temporal spectra of input, latent and reconstruction: each record gains "
                   "\"spectrum\" (three high-band shares, averaged over clips), each configuration a spectra_<config>.json")
    p.add_argument("--fps", type=float, default=None, help="with --spectrum: frame rate of the clips, adds the frequency axes; with "
                   "--save-yuv / --save-mjpeg: the rate written where the input file names none")
    p.add_argument("--content", action="store_true", help="content statistics of inputs and reconstructions: each record gains \"content\" "
                   "(inter- / intra-frame entropy, this project's definition, mean |difference|, TI, and the inter-frame entropy the "
                   "configuration removed)")
    p.add_argument("--bucket-dir", default=None, help="run the sweep once per <bucket>.txt list of this folder (tools/bucket_clips.py), "
                   "under <output-dir>/<bucket>/; records carry \"bucket\"")
    p.add_argument("--interp-mode", default=None, choices=INTERP_MODES, help="with --base-config: the interp_mode of every decoder block "
                   "of each enumerated configuration (default: what the base configuration says)")
    from hunyuanvideo_efficiency_amd.metrics import add_fvd_arguments, add_gssim_arguments, add_lpips_arguments
    add_gssim_arguments(p, csv=False)    # --gssim: each record gains "ssim3d", "ssim2d"
    from hunyuanvideo_efficiency_amd.metrics import add_motion_arguments, motion_from_args
    add_motion_arguments(p)              # --motion [--motion-block B] [--motion-radius R] [--motion-lam L]: each record gains "motion"
    add_lpips_arguments(p, synthetic=True)
    add_fvd_arguments(p)
    from hunyuanvideo_efficiency_amd.dataset import add_yuv_arguments, check_yuv_arguments
    add_yuv_arguments(p)
    from hunyuanvideo_efficiency_amd.video_io import add_save_yuv_argument
    add_save_yuv_argument(p)             # --save-yuv {y4m,I420,YV12,NV12}: under <output-dir>/recon_<config>/
    from hunyuanvideo_efficiency_amd.mjpeg_io import add_save_mjpeg_arguments, check_save_mjpeg_arguments
    add_save_mjpeg_arguments(p)          # --save-mjpeg [--save-quality Q] [--save-strip N]: <name>.avi, <name>_strip.jpg in the same folder
    from hunyuanvideo_efficiency_amd.mjpeg_io import add_mjpeg_input_arguments
    add_mjpeg_input_arguments(p)         # --mjpeg-input [--start-frame A] [--end-frame B]: --tensor-dir holds .avi files
    a = p.parse_args(argv)
    check_yuv_arguments(a, p)
    a.motion_params = motion_from_args(a, p)
    quality = check_save_mjpeg_arguments(p, a)
    a.mjpeg_params = dict(quality=quality, strip=a.save_strip) if a.save_mjpeg else None
    if a.fps is not None and not ((a.spectrum or a.save_yuv or a.save_mjpeg) and a.fps > 0):
        p.error("--fps needs --spectrum, --save-yuv or --save-mjpeg and a positive rate")
    if (a.base_config is None) == (a.config_dir is None):
        p.error("give exactly one of --base-config (enumerate) or --config-dir (ready-made configurations)")
    if a.interp_mode is not None and a.base_config is None:
        p.error("--interp-mode rewrites enumerated configurations: it needs --base-config")
    if a.lpips_linear and not a.lpips_alexnet:
        p.error("--lpips-linear needs --lpips-alexnet")
    if a.lpips_synthetic and a.lpips_alexnet:
        p.error("--lpips-synthetic and --lpips-alexnet exclude each other")
    if a.fvd_i3d and a.fvd_synthetic:
        p.error("--fvd-synthetic and --fvd-i3d exclude each other")
    if a.bucket_dir is not None and not os.path.isdir(a.bucket_dir):
        p.error(f"--bucket-dir {a.bucket_dir} is not a folder")
    return a


def main(argv=None):
    a = parse_args(argv)
    from hunyuanvideo_efficiency_amd.metrics import fvd_from_args, lpips_from_args
    lpips = lpips_from_args(a)
    fvd = fvd_from_args(a)
    input_logits = {}
    import dynamic_enumeration
    from infer import VideoTensorDataset
    os.makedirs(a.output_dir, exist_ok=True)
    if a.base_config:
        configs = dynamic_enumeration.write_configs(a.base_config, os.path.join(a.output_dir, f"config_{a.mode}_json"), a.mode, a.limit)
        if a.interp_mode is not None:
            override_interp_mode(configs, a.interp_mode)
    else:
        configs = [os.path.join(a.config_dir, f) for f in sorted((f for f in os.listdir(a.config_dir) if f.endswith(".json")), key=_exp_order)]
        configs = configs[:a.limit] if a.limit is not None else configs
    if a.yuv_format or a.mjpeg_input:
        from hunyuanvideo_efficiency_amd.dataset import dataset_from_args
        dataset = ConvertedOnce(dataset_from_args(a, "cuda"))
    else:
        dataset = VideoTensorDataset(a.tensor_dir)
    if a.bucket_dir is None:
        return run_sweep(a, configs, dataset, a.output_dir, lpips, fvd, input_logits, {} if a.content else None,
                         input_motion={} if a.motion_params else None)
    records = []
    for bucket, indices in read_bucket_lists(a.bucket_dir, dataset.tensor_files):
        print(f"bucket {bucket}: {len(indices)} clips")
        sub_dir = os.path.join(a.output_dir, bucket)
        os.makedirs(sub_dir, exist_ok=True)
        # the caches are keyed by the position in the subset: one pair per bucket
        records += run_sweep(a, configs, ClipSubset(dataset, indices), sub_dir, lpips, fvd, {}, {} if a.content else None, bucket,
                             {} if a.motion_params else None)
    return records


def run_sweep(a, configs, dataset, output_dir, lpips, fvd, input_logits, input_content, bucket=None, input_motion=None):
    """every configuration on `dataset` -> <output_dir>/study.jsonl; `bucket`: the label every record carries"""
    out =os.path.join(output_dir, "study.jsonl")
    records = []
    for cfg in configs:
        spectra = {} if a.spectrum else None
        rec = run_config(cfg, dataset, a.vae_path, a.reduced, "cuda", a.max_files, lpips, spectra, a.fps, fvd, input_logits, input_content, a.gssim,
                         a.save_yuv, os.path.join(output_dir, f"recon_{os.path.splitext(os.path.basename(cfg))[0]}"),
                         getattr(a, "motion_params", None), input_motion, getattr(a, "mjpeg_params", None))
        if bucket is not None:
            rec["bucket"] = bucket
        if spectra:
            with open(os.path.join(output_dir, f"spectra_{os.path.splitext(os.path.basename(cfg))[0]}.json"), "w") as f:
                json.dump(spectra, f)
        records.append(rec)
        with open(out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
    print(f"{len(records)} configurations -> {out}")
    return records


if __name__ == "__main__":
    main()
