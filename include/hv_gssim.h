/* Gaussian-window SSIM: the entry points of csrc/hv_gssim.hip in libhv_kernels.so, under the conventions of include/hv_kernels.h (plain
 * pointers + sizes + a hipStream_t, caller-owned buffers, 0 = HV_OK, -1 = bad argument before anything is enqueued, -2 = launch failure; a
 * host query returns 0 for every shape its kernel refuses).  They are declared here and not in hv_kernels.h: that header and its
 * HV_ABI_VERSION stay as they are (these are new symbols only), and this header has its own contract table (tests/gssim_contract.py,
 * checked without a GPU by tests/test_gssim_refusals_cpu.py).  The Python side parses this file as it parses hv_kernels.h
 * (hunyuanvideo_efficiency_amd/_abi.py: GSSIM_DECLS, GSSIM_MACROS); csrc/hv_gssim_torch_ops.cpp, generated from it by
 * tools/gen_torch_ops.py, registers torch.ops.hv.gaussian_ssim and gaussian_ssim_workspace_bytes. */
#ifndef HV_GSSIM_H
#define HV_GSSIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* SSIM of two videos under a separable HV_GSSIM_WIN-tap window, valid positions only: the measure of the fork's
 * rebuttal/common_metrics_on_video_quality (run.py: pytorch_msssim.ssim on [B,C,T,H,W], the window over T, H and W; calculate_ssim.py: the
 * same window per frame over H and W).
 * a, b [C,T,H,W] as hv_video_metrics reads its videos: dtype 0 = fp16, 1 = fp32; element strides *_sc, *_st, *_sh, W contiguous; every
 * element quantised to the byte save_videos_grid would write (the quantiser of hv_video_metrics, `rescale`).  win: the 11 weights, doubles
 * on the device.  temporal = 1: the window runs along T, H and W, To = T - 10 output frames; temporal = 0: along H and W, To = T.
 * ssim_sum: double [To][C], ssim_sum[t][c] = the sum of the SSIM map over the (H - 10) * (W - 10) positions of output frame t, channel c.
 * Every cell is written; row t depends on the input frames t .. t + 10 only (temporal = 0: on frame t alone), not on T.
 *
 * Arithmetic, all fp64, in code units (x, y in 0 .. 255; C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2 - the map is the one on codes / 255
 * with C1 = 0.01^2, C2 = 0.03^2).  Five fields x, y, x x, y y, x y (products of integers: exact) are filtered one axis after the other
 * in the order T (temporal = 1 only), H, W.  Each 1-D pass is the chain
 *     acc = win[0] * v[0];  acc = fma(win[k], v[k], acc) for k = 1 .. 10 in this order            (v[k] = the value k steps along the axis),
 * 11 roundings a pass.  With m1, m2, e11, e22, e12 the filtered fields:
 *     s1 = e11 - m1 m1, s2 = e22 - m2 m2, s12 = e12 - m1 m2       (each product rounded, then the difference; no contraction is relied on),
 *     map = ((2 m1 m2 + C1) / (m1 m1 + m2 m2 + C1)) * ((2 s12 + C2) / (s1 + s2 + C2)),  both divisions IEEE.
 * There is no constant-frame special case and no per-frame data range.
 * Sums: a workgroup owns a tile of HV_GSSIM_TILE_H x HV_GSSIM_TILE_W map positions of one channel and walks T; per output frame its 256
 * threads add their (at most two) map values, the lanes of a wave are folded by a fixed butterfly, the four waves in order; the tile
 * partial goes to `workspace` ([tile][To][C] doubles; >= hv_gaussian_ssim_workspace_bytes(C, T, H, W, temporal) bytes =
 * ceil((H - 10) / HV_GSSIM_TILE_H) * ceil((W - 10) / HV_GSSIM_TILE_W) * To * C * 8, 8-byte aligned) and a second kernel adds the tiles of a
 * cell in row-major tile order: no atomics, two runs give the same bits.  The filtered fields never reach memory.
 * HV_ERR_ARG (nothing launched, outputs untouched; the workspace query returns 0 for the shapes among them): H or W < HV_GSSIM_WIN or
 * > 65536; C other than 1 | 3; T < 1 or > 65535; temporal = 1 with T < HV_GSSIM_WIN; dtype, rescale or temporal other than 0 | 1;
 * negative or overlapping strides (sc, st < 0, sh < W); a, b, win, ssim_sum or workspace NULL; win, ssim_sum or workspace not 8-byte
 * aligned; a workspace that is too small. */
#define HV_GSSIM_WIN 11
#define HV_GSSIM_TILE_H 16
#define HV_GSSIM_TILE_W 32
int hv_gaussian_ssim(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st, int64_t b_sh,
                     int dtype, int C, int T, int H, int W, int rescale, int temporal, const double* win, double* ssim_sum,
                     void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t hv_gaussian_ssim_workspace_bytes(int C, int T, int H, int W, int temporal);

#ifdef __cplusplus
}
#endif
#endif /* HV_GSSIM_H */
