"""GPU: batch generation (several videos per call) through the product kernels.  Property: a batch adds no numerics of its own.
Video i of a batch - its per-step noise predictions, its latents and its decoded frames - equals, bit for bit, the single-video
call with generator[i] (the DiT and the VAE take the videos one after another through the same kernels and workspaces), and the
classifier-free-guidance batch [uncond x B*N | cond x B*N] matches the oracle per video.  The VAE decodes / reconstructs B videos
like B single-video calls on every path (concurrent tile streams, untiled, tile-parallel over ranks), and the drivers
(sample_video.py --num-videos, infer.py --batch-size) write one output per video."""
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from hunyuanvideo_efficiency_amd import synthetic as syn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BOC = (32, 64, 128, 128)


def _f16(t):
    return t.to(torch.float16).to(DEV)


def _record_noise_pred(model):
    """Forward hook on the DiT: every step's model output (the noise prediction of each row of the batch)."""
    rec = []
    model.register_forward_hook(lambda m, args, out: rec.append((out["x"] if isinstance(out, dict) else out).clone()))
    return rec


def _tiled_vae(**kw):
    from hunyuanvideo_efficiency_amd.vae import AutoencoderKLCausal3D
    vae = AutoencoderKLCausal3D(block_out_channels=BOC, sample_size=128, sample_tsize=16, device=DEV, **kw)
    vae.load_state_dict({k: v.to(torch.float16) for k, v in syn.synth_vae_state_dict(BOC, seed=0, encoder=kw.get("with_encoder", False)).items()},
                        strict=True)
    return vae


def test_one_prompt_three_videos_equal_single_video_runs():
    """(a) tiny DiT + reduced tiled VAE, 3 steps, num_videos_per_prompt=3, seed s: video i == the single-video run with seed s + i
    (noise prediction at every step, latents after every step, decoded frames)."""
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.diffusion.schedulers import FlowMatchDiscreteScheduler
    from hunyuanvideo_efficiency_amd.diffusion.pipelines import HunyuanVideoPipeline
    from hunyuanvideo_efficiency_amd.inference import get_rotary_pos_embed, resolve_seeds, seed_generators
    cfg = syn.tiny_config()
    model = build_model(cfg, DEV, seed=0)
    noise_preds = _record_noise_pred(model)
    pipe = HunyuanVideoPipeline(_tiled_vae(), model, FlowMatchDiscreteScheduler(shift=7.0, reverse=True, solver="euler"),
                                types.SimpleNamespace())
    frames, height, width, n_steps, s, n = 21, 192, 160, 3, 1234, 3       # 21 x 192 x 160: temporal AND spatial tiles, 2 streams
    lt, lh, lw = (frames - 1) // 4 + 1, height // 8, width // 8
    _, ts, tm, ts2 = syn.synth_dit_inputs(cfg, (lt, lh, lw), 32, 11, seed=3)
    freqs = get_rotary_pos_embed(model, frames, height, width, "884-16c-hy", 256, device=DEV)
    kw = dict(height=height, width=width, video_length=frames, num_inference_steps=n_steps, embedded_guidance_scale=6.0,
              freqs_cis=freqs, enable_tiling=True, n_tokens=freqs[0].shape[0], callback_steps=1)

    def run(num, gen):
        lats = []
        noise_preds.clear()
        v = pipe(_f16(ts), tm.to(DEV), _f16(ts2), num_videos_per_prompt=num, generator=gen,
                 callback=lambda i, t, lat: lats.append(lat.clone()), **kw).videos
        return v, lats, list(noise_preds)
    seeds = resolve_seeds(s, 1, n)
    assert seeds == [s, s + 1, s + 2]
    vb, lb, nb = run(n, seed_generators(seeds, DEV))
    assert vb.shape == (n, 3, frames, height, width) and len(lb) == len(nb) == n_steps
    for i in range(n):
        v1, l1, n1 = run(1, torch.Generator(DEV).manual_seed(s + i))
        for k in range(n_steps):
            assert torch.equal(nb[k][i:i + 1], n1[k]), ("noise_pred", i, k)
            assert torch.equal(lb[k][i:i + 1], l1[k]), ("latents", i, k)
        assert torch.equal(vb[i:i + 1], v1), ("frames", i)
    assert float((vb[0] - vb[1]).abs().max()) > 0.05 and float((vb[1] - vb[2]).abs().max()) > 0.05      # different seeds, videos


def test_cfg_two_prompts_two_videos_each_vs_single_runs_and_oracle():
    """(b) non-distilled model, guidance 3.5: two pre-computed prompts with 11 and 37 valid text tokens, 2 videos each (CFG batch of 8).
    Every video == its own single-video run bit for bit, and == the oracle's single-sample run within the bar of
    test_gpu_pipeline.py::test_pipeline_classifier_free_guidance_batch_vs_oracle."""
    from hunyuanvideo_efficiency_amd.builders import build_model
    from hunyuanvideo_efficiency_amd.diffusion.schedulers import FlowMatchDiscreteScheduler
    from hunyuanvideo_efficiency_amd.diffusion.pipelines import HunyuanVideoPipeline
    from hunyuanvideo_efficiency_amd.inference import get_rotary_pos_embed, resolve_seeds, seed_generators
    from oracle import dit_ref as RD
    cfg = syn.tiny_config()
    cfg.guidance_embed = False
    model = build_model(cfg, DEV, seed=0)
    pipe = HunyuanVideoPipeline(None, model, FlowMatchDiscreteScheduler(shift=7.0, reverse=True, solver="euler"), types.SimpleNamespace())
    frames, height, width, n_steps, scale = 17, 128, 128, 2, 3.5
    lt, lh, lw = (frames - 1) // 4 + 1, height // 8, width // 8
    prompts = [syn.synth_dit_inputs(cfg, (lt, lh, lw), 48, nv, seed=sd)[1:] for sd, nv in ((5, 11), (7, 37))]
    negs = [syn.synth_dit_inputs(cfg, (lt, lh, lw), 48, 4, seed=6)[1:]] * 2              # one negative prompt, 4 valid tokens
    cat = lambda parts, k: torch.cat([p[k] for p in parts])
    freqs = get_rotary_pos_embed(model, frames, height, width, "884-16c-hy", 256, device=DEV)
    kw = dict(height=height, width=width, video_length=frames, num_inference_steps=n_steps, embedded_guidance_scale=None, freqs_cis=freqs,
              output_type="latent", n_tokens=freqs[0].shape[0], guidance_scale=scale)
    seeds = resolve_seeds([40, 90], 2, 2)
    assert seeds == [40, 41, 90, 91]
    got = pipe(_f16(cat(prompts, 0)), cat(prompts, 1).to(DEV), _f16(cat(prompts, 2)), num_videos_per_prompt=2,
               generator=seed_generators(seeds, DEV), negative_prompt_embeds=_f16(cat(negs, 0)),
               negative_prompt_mask=cat(negs, 1).to(DEV), negative_prompt_embeds_2=_f16(cat(negs, 2)), **kw).videos
    assert got.shape == (4, 16, lt, lh, lw)
    E = RD.Prec(True)
    sd = {k: p.float().cpu() for k, p in model.state_dict().items()}
    cos, sin = RD.rope_tables([lt, lh // 2, lw // 2], cfg.rope_dim_list, 256.0)
    sig = RD.flow_sigmas(n_steps, 7.0)
    tsteps = RD.flow_timesteps(sig)
    h = lambda t: t.to(torch.float16).float()
    nts, ntm, nts2 = negs[0]
    for i, seed in enumerate(seeds):
        ts, tm, ts2 = prompts[i // 2]
        one = pipe(_f16(ts), tm.to(DEV), _f16(ts2), generator=torch.Generator(DEV).manual_seed(seed), negative_prompt_embeds=_f16(nts),
                   negative_prompt_mask=ntm.to(DEV), negative_prompt_embeds_2=_f16(nts2), **kw).videos
        assert torch.equal(got[i:i + 1], one), ("video", i)
        # oracle: the same initial noise (the pipeline draws fp16 latents from this video's generator), branches run separately
        lat = torch.randn((1, 16, lt, lh, lw), generator=torch.Generator(DEV).manual_seed(seed), device=DEV, dtype=torch.float16).float().cpu()
        for k in range(n_steps):
            vu = RD.dit_forward(sd, cfg, lat, tsteps[k:k + 1], h(nts), ntm, h(nts2), cos, sin, None, E).to(torch.bfloat16)
            vc = RD.dit_forward(sd, cfg, lat, tsteps[k:k + 1], h(ts), tm, h(ts2), cos, sin, None, E).to(torch.bfloat16)
            lat = RD.euler_step(lat, (vu + scale * (vc - vu)).float(), sig, k)
        ref = (lat / 2 + 0.5).clamp(0, 1)
        err = (got[i:i + 1] - ref).abs()
        assert float(err.max()) < 6e-2 and float(err.mean()) < 4e-3, (i, float(err.max()), float(err.mean()))
    assert float((got[0] - got[1]).abs().max()) > 0.05 and float((got[1] - got[2]).abs().max()) > 0.05


def test_vae_decode_and_forward_batch_equal_single_videos():
    """(c) decode of a B = 2 latent == two B = 1 decodes, tiled (two streams) and untiled; forward (encode -> mode -> decode) too."""
    vae = _tiled_vae(with_encoder=True)
    z = (syn.hashed_uniform((2, 16, 6, 24, 20), "batch.vae.z", 5) * 2.0).to(DEV)
    for tiled in (True, False):
        vae.enable_tiling(tiled)
        both = vae.decode(z, return_dict=False)[0]
        assert both.shape == (2, 3, 21, 192, 160)
        for b in range(2):
            assert torch.equal(both[b:b + 1], vae.decode(z[b:b + 1], return_dict=False)[0]), (tiled, b)
        vae.enable_slicing()                 # still accepted; same result
        assert torch.equal(vae.decode(z, return_dict=False)[0], both)
        vae.disable_slicing()
    assert float((both[0].float() - both[1].float()).abs().max()) > 0
    vae.disable_tiling()
    x = (syn.hashed_uniform((2, 3, 9, 64, 48), "batch.vae.x", 6)).to(DEV, torch.float16)
    rec, post = vae(x, return_dict=False, return_posterior=True)
    assert rec.shape == (2, 3, 9, 64, 48) and post.mode().shape[0] == 2
    for b in range(2):
        assert torch.equal(rec[b:b + 1], vae(x[b:b + 1], return_dict=False)[0]), ("forward", b)


def test_infer_driver_batch_size_two(tmp_path):
    """(c) infer.py --batch-size 2 on two .pt tensors: the same two reconstructions as --batch-size 1."""
    src = tmp_path / "in"
    src.mkdir()
    for i in range(2):
        torch.save(syn.hashed_uniform((3, 9, 64, 48), f"batch.infer.{i}", 7), src / f"clip{i}.pt")
    import importlib.util
    spec = importlib.util.spec_from_file_location("hv_infer", os.path.join(ROOT, "infer.py"))
    infer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(infer)
    outs = {}
    for bs in (1, 2):
        done = infer.main(["--tensor-dir", str(src), "--output-dir", str(tmp_path / f"out{bs}"), "--reduced", "--batch-size", str(bs)])
        assert len(done) == 2
        outs[bs] = [torch.load(tmp_path / f"out{bs}" / f"clip{i}.pt", weights_only=True) for i in range(2)]
    for i in range(2):
        assert outs[2][i].shape == (1, 3, 9, 64, 48)
        assert torch.equal(outs[1][i], outs[2][i]), i


def _tp_batch_worker(rank, world, port, outdir):
    """Tile-parallel VAE decode of a batch of 2 (every rank steps through the videos in the same order) == single-rank decodes."""
    sys.path.insert(0, ROOT)
    result = "FAIL: no result"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from tests.sp_gpu_helpers import stage_collectives_through_host
        stage_collectives_through_host()
        vae = _tiled_vae()
        vae.enable_tiling()
        z = (syn.hashed_uniform((2, 16, 6, 24, 20), "batch.vae.tp", 5) * 2.0).cuda()
        base = [vae.decode(z[b:b + 1], return_dict=False)[0].clone() for b in range(2)]
        vae.enable_tile_parallel()
        out = vae.decode(z, return_dict=False)[0]
        torch.cuda.synchronize()
        assert out.shape == (2, 3, 21, 192, 160)
        for b in range(2):
            assert torch.equal(out[b:b + 1], base[b]), b
        result = "ok"
    except Exception:  # noqa: BLE001
        import traceback
        result = "FAIL: " + traceback.format_exc()
    finally:
        with open(os.path.join(outdir, f"rank{rank}.txt"), "w") as f:
            f.write(result)
        dist.destroy_process_group()


def test_tile_parallel_vae_decode_batch_on_one_card(tmp_path):
    world = 2
    port = 29960 + (os.getpid() % 30)
    mp.start_processes(_tp_batch_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True, start_method="forkserver")
    results = {r: open(tmp_path / f"rank{r}.txt").read() for r in range(world)}
    assert all(v == "ok" for v in results.values()), results


def _read_frames(path):
    import numpy as np
    if path.endswith(".npy"):
        return np.load(path)
    if path.endswith(".gif"):
        from PIL import Image, ImageSequence
        with Image.open(path) as im:
            return np.stack([np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)])
    import imageio
    return np.stack(imageio.mimread(path))


def test_sample_video_cli_two_videos(tmp_path):
    """(d) sample_video.py --tiny --num-videos 2 --seed 7 in a fresh process: two files named with seeds 7 and 8, different frames."""
    out = tmp_path / "results"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "sample_video.py"), "--tiny", "--infer-steps", "2", "--num-videos", "2",
                        "--seed", "7", "--video-size", "64", "64", "--video-length", "5", "--flow-reverse", "--save-path", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert len(files) == 2 and files[0].startswith("seed7_synthetic.") and files[1].startswith("seed8_synthetic."), files
    f7, f8 = (_read_frames(str(out / f)) for f in files)
    assert f7.shape[1:] == f8.shape[1:] == (64, 64, 3), (f7.shape, f8.shape)
    assert (f7[0] != f8[0]).any()          # first frames differ: each video has its own noise
