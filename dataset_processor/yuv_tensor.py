#!/usr/bin/env python3
"""Raw planar YUV 4:2:0 files -> `.pt` video tensors, the fork's dataset_processor/yuv_tensor.py on the MI355X kernel
(csrc/hv_yuv.hip): for every `<name>_<n>fps_<w>x<h>.yuv` of --video-dir write --output-dir/<name>_..._.pt, an fp32 [3,T,H,W] tensor in
[-1, 1], and print a per-file summary.  The fork's flags --target_height, --start_frame, --end_frame and --yuv_format are kept;
--video-dir and --output-dir are new, because the fork hard-codes its paths.

Differences to the fork, on purpose:
  * With --target_height the fork's `.pt` stays at SOURCE size and only its mp4 is resized; the resized frames reach a tensor through
    mp42tensor.py, after an mp4v encode.  Here the TENSOR is resized: the one-step form of yuv_tensor.py followed by mp42tensor.py,
    without the codec in between.  The resize is this project's own 2-tap bilinear rule (include/hv_kernels.h), not cv2.resize's bytes.
  * No mp4 is written.
  * The colour conversion restates OpenCV's fixed-point BT.601 rule; cv2 is not part of this environment, so it is not pinned against
    it (tests/test_yuv_cpu.py holds the independent anchors).

  python dataset_processor/yuv_tensor.py --video-dir D --output-dir O [--yuv_format I420|NV12|YV12] [--target_height 240]
                                         [--start_frame A] [--end_frame B]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Raw YUV 4:2:0 files to video tensors (MI355X kernel).")
    p.add_argument("--target_height", type=int, default=None, help="rows of the output (e.g. 720 / 360 / 240); default: source size")
    p.add_argument("--start_frame", type=int, default=None, help="first frame (inclusive); default 0")
    p.add_argument("--end_frame", type=int, default=None, help="last frame (exclusive); default: the last whole frame of the file")
    p.add_argument("--yuv_format", type=str, default="I420", choices=["I420", "NV12", "YV12"], help="layout of the input files")
    p.add_argument("--video-dir", type=str, required=True, help="folder of .yuv files")
    p.add_argument("--output-dir", type=str, required=True, help="where the .pt tensors go")
    a = p.parse_args(argv)
    if a.target_height is not None and a.target_height < 1:
        p.error("--target_height must be positive")
    if (a.start_frame is not None and a.start_frame < 0) or (a.end_frame is not None and a.end_frame < 0):
        p.error("--start_frame and --end_frame are non-negative")
    return a


def main(argv=None):
    a = parse_args(argv)
    import torch
    from hunyuanvideo_efficiency_amd.dataset import YuvClipDataset, parse_yuv_name
    os.makedirs(a.output_dir, exist_ok=True)
    dataset = YuvClipDataset(a.video_dir, "cuda", a.yuv_format, a.start_frame, a.end_frame, a.target_height, dtype=torch.float32)
    if not len(dataset) and not dataset.skipped:
        print(f"No .yuv files in {a.video_dir}")
    done = []
    for idx in range(len(dataset)):
        clip, name = dataset[idx]
        _, width, height = parse_yuv_name(name)
        path = os.path.join(a.output_dir, name[:-len(".yuv")] + ".pt")
        video = clip.cpu()
        torch.save(video, path)
        C, T, H, W = video.shape
        print("=" * 50)
        print(f"Processed: {name}\n"
              f"  source size: {width}x{height}\n"
              f"  output size: {W}x{H}\n"
              f"  tensor shape: C={C}, T={T}, H={H}, W={W}\n"
              f"  value range: [-1, 1], dtype={video.dtype}")
        done.append(path)
    print(f"{len(done)} files converted")
    return done


if __name__ == "__main__":
    main()
