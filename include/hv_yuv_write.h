/* Video tensor -> raw YUV 4:2:0 frames: the entry point of csrc/hv_yuv_write.hip in libhv_kernels.so, under the conventions of
 * include/hv_kernels.h (plain pointers + sizes + a hipStream_t, caller-owned buffers, 0 = HV_OK, -1 = bad argument before anything is
 * enqueued, -2 = launch failure).  It is the mirror image of hv_yuv420_to_clip.  It is declared here and not in hv_kernels.h: that header
 * and its HV_ABI_VERSION stay as they are (this is a new symbol only), and this header has its own contract table
 * (tests/yuv_write_contract.py, checked without a GPU by tests/test_yuv_write_refusals_cpu.py).  The Python side parses this file as it
 * parses hv_kernels.h (hunyuanvideo_efficiency_amd/_abi.py: YUVW_DECLS, YUVW_MACROS); csrc/hv_yuv_write_torch_ops.cpp, generated from it by
 * tools/gen_torch_ops.py, registers torch.ops.hv.clip_to_yuv420. */
#ifndef HV_YUV_WRITE_H
#define HV_YUV_WRITE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* x [C,T,H,W] as hv_video_metrics reads a video: dtype 0 = fp16, 1 = fp32; element strides sc, st, sh, W contiguous; C = 1 | 3, a gray
 * input gives R = G = B.  x is only read: strides may overlap (an expanded view with st == 0 is legal) but not be negative.
 *
 * Quantiser.  Every element becomes the byte save_videos_grid would write (utils/file_utils.py:frames_uint8, the quantiser of
 * hv_video_metrics): v = float(x); if rescale: v = (v + 1.0) / 2.0; v = clamp(v, 0, 1); q = (uint8)(v * 255.0), every step rounded to
 * fp32 on its own, the last one truncating; NaN gives 0.
 *
 * Colour.  BT.601 limited range in 20 fractional bits on the bytes R, G, B, int32, `>>` arithmetic:
 *     Y = ( 269484 R + 528482 G + 102760 B + (16  << 20) + 2^19) >> 20        per pixel
 *     U = (-155188 R - 305135 G + 460324 B + (128 << 20) + 2^19) >> 20
 *     V = ( 460324 R - 385875 G -  74448 B + (128 << 20) + 2^19) >> 20
 * No clamp: Y lies in 16 .. 235 and U, V in 16 .. 240 for every byte triple.  UNPINNED RESTATEMENT: this is OpenCV's COLOR_RGB2YUV_I420
 * rule as far as it can be established without running it; cv2 cannot be executed here, so parity with its bytes is not claimed.
 *
 * Chroma of the 2 x 2 block of pixels (2r .. 2r + 1, 2c .. 2c + 1) -> sample (r, c):
 *     chroma = 0   U, V of the block's top-left pixel by the formulas above (as OpenCV does);
 *     chroma = 1   with Rs, Gs, Bs the sums of the four pixels' bytes,
 *                      U = (-155188 Rs - 305135 Gs + 460324 Bs + (128 << 22) + 2^21) >> 22,
 *                      V = ( 460324 Rs - 385875 Gs -  74448 Bs + (128 << 22) + 2^21) >> 22
 *                  (fits int32) - THIS PROJECT'S rule, centre-sited; same range.
 *
 * Output.  raw: T frames at a pitch of W * H * 3 / 2 bytes, Y [H][W] first, then by `layout` (the values of HV_YUV_I420 = 0,
 * HV_YUV_YV12 = 1, HV_YUV_NV12 = 2 of hv_kernels.h): I420: U [H/2][W/2], V [H/2][W/2]; YV12: V, U; NV12: [H/2][W/2] interleaved (U, V)
 * pairs.  Frame offsets are 64-bit; every output byte is written exactly once; no atomics: two runs give the same bytes.
 *
 * HV_ERR_ARG, nothing launched: x or raw NULL; odd or non-positive W or H; a side above HV_YUV_MAX_SIDE (16384, hv_kernels.h); T < 1;
 * C other than 1 | 3; dtype, rescale or chroma other than 0 | 1; an unknown layout; x not aligned to its dtype; a negative stride. */
#define HV_YUVW_CHROMA_TOPLEFT 0
#define HV_YUVW_CHROMA_MEAN 1
int hv_clip_to_yuv420(const void* x, int dtype, int C, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, int rescale, int layout,
                      int chroma, void* raw, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HV_YUV_WRITE_H */
