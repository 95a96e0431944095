#!/usr/bin/env python3
"""Sort the clips of a folder into content buckets by inter-frame entropy, on the GPU: the lists the fork's run_experiments_buckets.sh
reads (metric_buckets/InterEntropy_buckets/Very_Low_InterEntropy_lt2.txt, Low_InterEntropy_2-4.txt, Medium_InterEntropy_4-6.txt), plus
High_InterEntropy_gt6 for what lies above its last edge.  The fork publishes the bucket names and edges, not the program that computed the
measure: the definition here - the Shannon entropy, in bits, of the histogram of the difference of consecutive 8-bit gray frames, averaged
over the frame pairs of a clip - is this project's own (metrics.content_entropy; every record carries it as "definition").

  python tools/bucket_clips.py --tensor-dir D --output-dir O [--metric inter|intra] [--edges 2 4 6] [--max-files N]
  ... --yuv-format I420 [--target-height 240] [--start-frame A] [--end-frame B]   D is a folder of raw planar YUV 4:2:0 files

Writes O/content.jsonl (one record per clip: "file", "name", the fields of metrics.content_entropy, "metric", "value", "bucket") and one
list per non-empty bucket, O/<bucket>.txt, the input paths one per line, sorted; prints one line per bucket.  Buckets are half-open,
[lo, hi): exactly 2.0 is Low.  A single-frame clip has no inter-frame entropy: its record has "bucket": null and it is in no list.
All clips are enqueued before the one host synchronisation.  tools/run_vae_study.py --bucket-dir O then runs the sweep per list.

  ... --metric motion --edges E1 [E2 ...] [--motion-block 8|16] [--motion-radius R] [--motion-lam L]
sorts by how much a clip moves instead (the fork's dataset tool reads a folder called `large_motion`; it does not say how the clips got
there): `motion_mean` of metrics.motion_stats, the mean length in px/frame of the block-matching vectors - this project's own measure, not
FVMD.  Nobody has measured natural clips under this definition, so --edges has no default here; the records go to O/motion.jsonl and the
lists are named <rank>_Motion_<span>.txt."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Content buckets of a clip folder by inter-frame entropy (this project's definition).")
    p.add_argument("--tensor-dir", required=True, help="input .pt video tensors [C,T,H,W] (or .yuv files with --yuv-format)")
    p.add_argument("--output-dir", required=True, help="content.jsonl and the <bucket>.txt lists go here")
    p.add_argument("--metric", choices=("inter", "intra", "motion"), default="inter", help="bucket by the entropy of the frame difference "
                   "(default), of the gray frame itself, or by the mean block-matching motion in px/frame (needs --edges)")
    p.add_argument("--edges", type=float, nargs="+", default=None, help="ascending bucket edges, in bits (default: the fork's 2 4 6) or, "
                   "with --metric motion, in px/frame (no default)")
    from hunyuanvideo_efficiency_amd import metrics
    p.add_argument("--motion-block", type=int, default=None, choices=metrics.MOTION_BLOCKS, help="with --metric motion: block size (default 16)")
    p.add_argument("--motion-radius", type=int, default=None, help="with --metric motion: search radius (default 16)")
    p.add_argument("--motion-lam", type=int, default=None, help="with --metric motion: penalty per pixel of |dy| + |dx| (default block^2 // 16)")
    p.add_argument("--max-files", type=int, default=None)
    from hunyuanvideo_efficiency_amd.dataset import add_yuv_arguments, check_yuv_arguments
    add_yuv_arguments(p)
    a = p.parse_args(argv)
    check_yuv_arguments(a, p)
    a.motion = a.metric == "motion"
    sub = [f for f, v in (("--motion-block", a.motion_block), ("--motion-radius", a.motion_radius), ("--motion-lam", a.motion_lam)) if v is not None]
    if sub and not a.motion:
        p.error(f"{', '.join(sub)} only valid with --metric motion")
    a.motion_params = metrics.motion_from_args(a, p)
    if a.edges is None:
        if a.motion:
            p.error("--metric motion needs --edges in px/frame: nobody has measured natural clips under this definition, there is no default")
        a.edges = [2.0, 4.0, 6.0]
    if any(b <= e for e, b in zip(a.edges, a.edges[1:])):
        p.error(f"--edges must be ascending, got {a.edges}")
    if a.motion and any(not 0.0 < e < 2 ** 0.5 * a.motion_params["radius"] for e in a.edges):
        p.error(f"--edges are vector lengths in px/frame, between 0 and radius * sqrt(2), got {a.edges}")
    if not a.motion and any(not 0.0 < e < 16.0 for e in a.edges):
        p.error(f"--edges are entropies in bits, between 0 and 16, got {a.edges}")
    if a.max_files is not None and a.max_files < 1:
        p.error("--max-files must be positive")
    if not os.path.isdir(a.tensor_dir):
        p.error(f"--tensor-dir {a.tensor_dir} is not a folder")
    return a


def measure_on_gpu(dataset, n, device="cuda"):
    """metrics.content_entropy of the first n clips of `dataset`: a clip is loaded, its launches enqueued, and dropped; one synchronisation"""
    import torch
    from hunyuanvideo_efficiency_amd import metrics

    def clips():
        for idx in range(n):
            video, _ = dataset[idx]
            yield video.to(device, dtype=torch.float16)     # what the drivers feed the VAE
    return metrics.content_entropy_many(clips())


def motion_on_gpu(dataset, n, params, device="cuda"):
    """metrics.motion_stats of the first n clips of `dataset`, as `measure_on_gpu` takes the entropies: one synchronisation"""
    import torch
    from hunyuanvideo_efficiency_amd import metrics

    def clips():
        for idx in range(n):
            video, _ = dataset[idx]
            yield video.to(device, dtype=torch.float16)
    return metrics.motion_stats_many(clips(), **params)


def bucket_records(files, tensor_dir, stats, metric, edges):
    """file names and their content_entropy dicts -> (records, {bucket label: sorted paths})"""
    from hunyuanvideo_efficiency_amd import metrics
    from hunyuanvideo_efficiency_amd.dataset import clip_stem
    records, lists = [], {}
    for name, d in zip(files, stats):
        value = d[{"inter": "inter_entropy", "intra": "intra_entropy", "motion": "motion_mean"}[metric]]
        label = metrics.content_bucket(value, edges, metric)
        path = os.path.join(tensor_dir, name)
        records.append(dict(file=path, name=clip_stem(name), **d, metric=metric, value=value, bucket=label))
        if label is not None:
            lists.setdefault(label, []).append(path)
    return records, {k: sorted(v) for k, v in lists.items()}


def main(argv=None, measure=measure_on_gpu, measure_motion=motion_on_gpu):
    """`measure(dataset, n)` -> the content_entropy dict of each of the first n clips, `measure_motion(dataset, n, params)` -> the
    motion_stats dict of each (the tests pass numpy doubles)"""
    a = parse_args(argv)
    from hunyuanvideo_efficiency_amd import metrics
    if a.yuv_format:
        from hunyuanvideo_efficiency_amd.dataset import dataset_from_args
        dataset = dataset_from_args(a, "cuda")
    else:
        from infer import VideoTensorDataset
        dataset = VideoTensorDataset(a.tensor_dir)
    n = len(dataset) if a.max_files is None else min(len(dataset), a.max_files)
    if n == 0:
        raise SystemExit(f"no clips in {a.tensor_dir}")
    stats = measure_motion(dataset, n, a.motion_params) if a.motion else measure(dataset, n)
    records, lists = bucket_records(dataset.tensor_files[:n], a.tensor_dir, stats, a.metric, a.edges)
    os.makedirs(a.output_dir, exist_ok=True)
    jsonl = os.path.join(a.output_dir, "motion.jsonl" if a.motion else "content.jsonl")
    with open(jsonl, "w") as f:
        for r in records:
            f.write(json.dumps(r) + "\n")
    for label in metrics.content_bucket_labels(a.edges, a.metric):
        paths = lists.get(label)
        if not paths:
            continue
        with open(os.path.join(a.output_dir, label + ".txt"), "w") as f:
            f.write("".join(p + "\n" for p in paths))
        vals = [r["value"] for r in records if r["bucket"] == label]
        what = "motion" if a.motion else f"{a.metric}-frame entropy"
        unit = "px/frame" if a.motion else "bits"
        tail = "this project's own measure, not FVMD" if a.motion else "this project's definition"
        print(f"{label}: {len(paths)} clips, mean {what} {sum(vals) / len(vals):.4f} {unit} "
              f"[{min(vals):.4f}, {max(vals):.4f}] ({tail})")
    unbucketed = [r["name"] for r in records if r["bucket"] is None]
    if unbucketed:
        print(f"no bucket (a single frame has no inter-frame {'motion' if a.motion else 'entropy'}): {', '.join(unbucketed)}")
    print(f"{len(records)} clips -> {jsonl}")
    return records


if __name__ == "__main__":
    main()
