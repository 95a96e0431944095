/* Content statistics: the entry points of csrc/hv_content.hip in libhv_kernels.so, under the conventions of include/hv_kernels.h (plain
 * pointers + sizes + a hipStream_t, caller-owned buffers, 0 = HV_OK, -1 = bad argument before anything is enqueued, -2 = launch failure; a
 * host query returns 0 for every shape its kernel refuses).  They are declared here and not in hv_kernels.h: that header and its
 * HV_ABI_VERSION stay as they are (these are new symbols only; no existing signature or buffer layout changes), and this header has its
 * own contract table (tests/content_contract.py, checked without a GPU by tests/test_content_refusals_cpu.py).  The Python side parses
 * this file as it parses hv_kernels.h (hunyuanvideo_efficiency_amd/_abi.py: CONTENT_DECLS, CONTENT_MACROS);
 * csrc/hv_content_torch_ops.cpp, generated from it by tools/gen_torch_ops.py, registers torch.ops.hv.content_histograms,
 * content_histograms_workspace_bytes and histogram_entropy. */
#ifndef HV_CONTENT_H
#define HV_CONTENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* Content statistics of a clip (the measure behind the fork's metric_buckets/InterEntropy_buckets/ lists, run per bucket by
 * run_experiments_buckets.sh; the fork publishes the bucket names and edges, not the program, so the definition is this project's own):
 * histograms of the 8-bit gray frames of x [3,T,H,W] and of the differences of consecutive gray frames.  x as hv_temporal_spectrum reads
 * it in mode 0: dtype 0 = fp16, 1 = fp32; element strides sc, st, sh, W contiguous; R, G, B quantised to the byte save_videos_grid would
 * write (the quantiser of hv_video_metrics, `rescale`) and combined to the integer luma (wr R + wg G + wb B + round) >> shift, which must
 * stay a byte: weights and round >= 0, shift <= 22, weights <= 2^22, (wr + wg + wb) * 255 + round < 256 << shift.
 * intra: uint32 [T][256], intra[t][g] = pixels of frame t with gray value g.  inter: uint32 [T - 1][HV_CONTENT_INTER_BINS],
 * inter[t][d + 255] = pixels with gray[t + 1] - gray[t] == d.  T == 1: no inter rows, inter may be NULL and nothing is written there.
 * Every cell of both outputs is written (no initialisation by the caller); counts are exact integers (H * W <= 2^31 - 1 fits the word),
 * so two runs give the same bits and row t depends on its own frames only, not on T.  The gray frames never reach memory.
 * A workgroup counts HV_CONTENT_CHUNK pixels of a frame; its partial rows go to `workspace` (>= hv_content_histograms_workspace_bytes(T, H,
 * W) bytes = ceil(H * W / HV_CONTENT_CHUNK) * (T * 256 + (T - 1) * HV_CONTENT_INTER_BINS) * 4, 4-byte aligned) and are added in chunk
 * order: no global atomics.  T < 1, T > 65535, H or W outside [1, 65536], H * W above 2^31 - 1, negative or overlapping strides (sh < W)
 * are HV_ERR_ARG (the workspace query returns 0 for the shapes among them), as are dtype or rescale other than 0 | 1, a luma that can
 * leave the byte, intra or inter not 4-byte aligned, inter NULL with T > 1 and a workspace that is too small. */
#define HV_CONTENT_INTER_BINS 511
#define HV_CONTENT_CHUNK 8192
int hv_content_histograms(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int T, int H, int W, int rescale, int wr, int wg,
                          int wb, int round, int shift, void* intra, void* inter, void* workspace, int64_t workspace_bytes,
                          hipStream_t stream);
int64_t hv_content_histograms_workspace_bytes(int T, int H, int W);

/* Entropy and moments of histogram rows: counts uint32 [rows][bins] (4-byte aligned), bin b standing for the value b - origin ->
 * out double [rows][3] (8-byte aligned) = (Shannon entropy in bits, sum c v, sum c v^2).  One wave per row.  N = sum c and the two moments
 * are 64-bit integers, exact, and exact as doubles while below 2^53 (rows of hv_content_histograms: N <= 2^31 - 1, |v| <= 255, so below
 * 2^47).  Entropy = log2 N - (sum c log2 c) / N in fp64, lane l adding bins l, l + 64, ... in order, then a fixed butterfly; a zero count
 * adds 0; never below 0.  A row with N == 0 gives 0, 0, 0.  rows >= 0 (rows == 0: HV_OK, nothing done) and <= 2^31 - 1; 1 <= bins <= 1024;
 * 0 <= origin <= bins. */
int hv_histogram_entropy(const void* counts, int64_t rows, int bins, int origin, double* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HV_CONTENT_H */
