/* Block-matching motion fields: the entry point of csrc/hv_motion.hip in libhv_kernels.so, under the conventions of include/hv_kernels.h
 * (plain pointers + sizes + a hipStream_t, caller-owned buffers, 0 = HV_OK, -1 = bad argument before anything is enqueued, -2 = launch
 * failure).  It is declared here and not in hv_kernels.h: that header and its HV_ABI_VERSION stay as they are (a new symbol only; no
 * existing signature or buffer layout changes), and this header has its own contract table (tests/motion_contract.py, checked without a
 * GPU by tests/test_motion_refusals_cpu.py).  The Python side parses this file as it parses hv_kernels.h
 * (hunyuanvideo_efficiency_amd/_abi.py: MOTION_DECLS, MOTION_MACROS); csrc/hv_motion_torch_ops.cpp, generated from it by
 * tools/gen_torch_ops.py, registers torch.ops.hv.block_motion. */
#ifndef HV_MOTION_H
#define HV_MOTION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* Dense full-search block matching between consecutive 8-bit gray frames of a clip x [3,T,H,W].  THE MEASURE IS THIS PROJECT'S OWN: it
 * is not FVMD (the fork's `fvdm` column, keypoint tracks from a third-party tracker) and does not stand in for it.
 * x as hv_content_histograms reads it: dtype 0 = fp16, 1 = fp32; element strides sc, st, sh, W contiguous; R, G, B quantised to the byte
 * save_videos_grid would write (the quantiser of hv_video_metrics, `rescale`) and combined to the integer luma
 * g = (wr R + wg G + wb B + round) >> shift, which must stay a byte: weights and round >= 0, shift <= 22, weights <= 2^22,
 * (wr + wg + wb) * 255 + round < 256 << shift.  The gray frames never reach memory.
 * Blocks of block x block pixels (block = 8 | 16) tile frame t + 1 from (0, 0): Hb = ceil(H / block), Wb = ceil(W / block); edge blocks
 * are partial and sum over the pixels they have.  For pair t (frames t, t + 1), block (by, bx) and displacement (dy, dx) in
 * [-radius, radius]^2, 1 <= radius <= HV_MOTION_MAX_RADIUS:
 *   SAD(dy, dx) = sum |g[t + 1][y][x] - g[t][clamp(y + dy, 0, H - 1)][clamp(x + dx, 0, W - 1)]|     (replicated edges)
 *   cost        = SAD + lam * (|dy| + |dx|),  0 <= lam <= HV_MOTION_MAX_LAM
 * and the winner is the minimum under the lexicographic order (cost, dy^2 + dx^2, dy, dx): unique, a flat block gives (0, 0).
 * mv: int16 [T - 1][Hb][Wb][2] = (dy, dx), 4-byte aligned; sad: uint32 [T - 1][Hb][Wb] = the winner's SAD without the penalty; sad0:
 * uint32, same shape = the SAD at (0, 0); both 4-byte aligned.  Every cell is written (no initialisation by the caller); integers
 * throughout, no atomics: two runs give the same bits and pair t depends on its two frames only, not on T.  T == 1: no rows, the three
 * outputs may be NULL, nothing is enqueued and the call returns HV_OK.
 * A workgroup takes HV_MOTION_TILE x HV_MOTION_TILE pixels of frame t + 1; no workspace.
 * T < 1, T > 65535, H or W outside [1, 65536], H * W above 2^31 - 1, negative or overlapping strides (sh < W), dtype or rescale other
 * than 0 | 1, a luma that can leave the byte, block other than 8 | 16, radius outside [1, HV_MOTION_MAX_RADIUS], lam outside
 * [0, HV_MOTION_MAX_LAM], an output not 4-byte aligned and a NULL output with T > 1 are HV_ERR_ARG. */
#define HV_MOTION_TILE 32
#define HV_MOTION_MAX_RADIUS 32
#define HV_MOTION_MAX_LAM 255
int hv_block_motion(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int T, int H, int W, int rescale, int wr, int wg, int wb,
                    int round, int shift, int block, int radius, int lam, void* mv, void* sad, void* sad0, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HV_MOTION_H */
