// Dense full-search block matching between consecutive 8-bit gray frames of a clip on the device (include/hv_motion.h has the definition;
// the measure is this project's own, not FVMD).  The gray frames are those of hv_content.hip: quantise() (hv_common.hpp) on R, G, B, then
// the integer luma (wr R + wg G + wb B + round) >> shift.  They never reach HBM.
//
//   block_motion_kernel<T, B>  a workgroup of four waves owns kTile x kTile pixels of frame t + 1 (2 x 2 blocks of 16, 4 x 4 of 8) and
//                              stages, as gray bytes in LDS, that tile (pixels outside the frame as 0) and the (kTile + 2 R)^2 window of
//                              frame t around it with clamped coordinates, so neighbouring blocks share what their windows overlap and
//                              nothing outside the frame is read.  A wave then takes one block at a time: the block's rows go to
//                              registers (B / 4 dwords a row), lane l takes displacement dx = l mod (2 R + 1) and kDy consecutive dy.  A
//                              window row is read once per lane (B / 4 + 1 dwords, consecutive lanes one byte apart: four lanes share a
//                              dword, no bank conflicts), shifted to the lane's byte offset by v_alignbyte_b32, masked to the block's
//                              columns inside the frame, and differenced against the kDy block rows that meet it with v_sad_u8 - four
//                              byte differences an instruction, kDy * B / 4 of them for B / 4 + 1 LDS reads.  Rows below the frame are
//                              skipped by a wave-uniform branch.  Every candidate becomes the key (cost, dy^2 + dx^2, dy, dx) packed
//                              into 64 bits; a lane keeps its minimum, the wave's butterfly the block's.  One lane stores the winner, the
//                              lane that holds (0, 0) stores sad0: every cell has exactly one writer, plain vector stores, no atomics,
//                              integers throughout.  The time does not depend on the content (no early exit).
#include "hv_common.hpp"
#include "../../include/hv_motion.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = HV_MOTION_TILE;                      // pixels a side of a workgroup's part of frame t + 1
constexpr int kMaxR = HV_MOTION_MAX_RADIUS, kMaxLam = HV_MOTION_MAX_LAM;
constexpr int kDy = 4;                                     // consecutive dy of one lane: they share every window row it reads
constexpr int kWinRows = kTile + 2 * kMaxR + kDy - 1;      // the last lanes' dy beyond the radius read (and discard) kDy - 1 rows more
constexpr int kWinDwords = (kTile + 2 * kMaxR) / 4 + 1;    // a row and the dword the last aligned read runs into
constexpr int kMaxT = 65535;                               // pairs are grid.z
static_assert(kTile % 16 == 0 && kTile * kTile / 4 == kThreads, "one quad of the tile per thread; whole blocks of 8 and 16");
// the key: cost < 2^17 (256 * 255 + 255 * 2 * 32), norm <= 2 * 32^2 < 2^12, dy + kMaxR and dx + kMaxR < 2^7
static_assert(256 * 255 + kMaxLam * 2 * kMaxR < (1 << 17) && 2 * kMaxR * kMaxR < (1 << 12) && 2 * kMaxR < (1 << 7), "the packed key");

struct Luma {
    int wr, wg, wb, round, shift;
};

struct WaveMinU64 {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long a, unsigned long long b) const { return a < b ? a : b; }
};

template <typename T>
__device__ __forceinline__ uint32_t gray_at(const T* __restrict__ frame, int64_t sc, int64_t sh, int y, int x, int rescale, const Luma& lu) {
    const T* p = frame + (int64_t)y * sh + x;
    return (uint32_t)((lu.wr * (int)quantise((float)p[0], rescale) + lu.wg * (int)quantise((float)p[sc], rescale) +
                       lu.wb * (int)quantise((float)p[2 * sc], rescale) + lu.round) >> lu.shift);
}

template <typename T, int B>
__global__ __launch_bounds__(kThreads) void block_motion_kernel(const T* __restrict__ x, int64_t sc, int64_t st, int64_t sh, int H, int W,
                                                               int Hb, int Wb, int rescale, Luma lu, int R, int lam,
                                                               uint32_t* __restrict__ mv, uint32_t* __restrict__ sad,
                                                               uint32_t* __restrict__ sad0) {
    __shared__ uint32_t s_win[kWinRows * kWinDwords];
    __shared__ uint32_t s_cur[kTile * kTile / 4];
    constexpr int NB = kTile / B, W4 = B / 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.z, y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const int S4 = (kTile + 2 * R + 3) / 4 + 1;            // dwords of a window row: <= kWinDwords
    const int NR = kTile + 2 * R + kDy - 1;                // window rows: <= kWinRows
    const T* prev = x + (int64_t)pair * st;
    const T* cur = prev + st;

    for (int q = tid; q < NR * S4; q += kThreads) {        // the window of frame t, every coordinate clamped into the frame
        const int wr = q / S4, wq = q - wr * S4;
        const int y = min(max(y0 - R + wr, 0), H - 1);
        uint32_t g4 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = min(max(x0 - R + 4 * wq + i, 0), W - 1);
            g4 |= gray_at(prev, sc, sh, y, xx, rescale, lu) << (8 * i);
        }
        s_win[q] = g4;
    }
    {                                                      // the tile of frame t + 1: one quad per thread, 0 outside the frame
        const int y = y0 + tid / (kTile / 4), xq = x0 + 4 * (tid % (kTile / 4));
        uint32_t g4 = 0;
        if (y < H) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (xq + i < W) g4 |= gray_at(cur, sc, sh, y, xq + i, rescale, lu) << (8 * i);
        }
        s_cur[tid] = g4;
    }
    __syncthreads();

    const int n = 2 * R + 1, items = ((n + kDy - 1) / kDy) * n;       // an item = (group of kDy dy, dx)
    for (int b = wave; b < NB * NB; b += kWaves) {
        const int bby = b / NB, bbx = b % NB;
        const int by = blockIdx.y * NB + bby, bx = blockIdx.x * NB + bbx;
        if (by >= Hb || bx >= Wb) continue;                // wave-uniform; no barrier follows
        const int nrows = min(B, H - by * B);              // rows of the block inside the frame
        uint32_t c[B][W4], cm[W4];
#pragma unroll
        for (int r = 0; r < B; ++r)
#pragma unroll
            for (int j = 0; j < W4; ++j) c[r][j] = s_cur[(bby * B + r) * (kTile / 4) + bbx * W4 + j];
#pragma unroll
        for (int j = 0; j < W4; ++j) {                     // the block's columns inside the frame, a byte each
            cm[j] = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (bx * B + 4 * j + i < W) cm[j] |= 0xFFu << (8 * i);
        }
        const int64_t cell = ((int64_t)pair * Hb + by) * Wb + bx;
        unsigned long long best = ~0ull;
        for (int base = 0; base < items; base += 64) {
            const bool live = base + lane < items;
            const int it = live ? base + lane : 0;
            const int g = it / n, dxi = it - g * n;
            const int off = bbx * B + dxi;                 // byte offset of the lane's first window column
            const uint32_t* wp = s_win + (bby * B + kDy * g) * S4 + (off >> 2);
            const uint32_t shift = (uint32_t)(off & 3);
            uint32_t acc[kDy] = {};
#pragma unroll
            for (int wr = 0; wr < B + kDy - 1; ++wr) {     // window row wr meets block row wr - k for the lane's k-th dy
                if (wr - (kDy - 1) < nrows) {
                    uint32_t v[W4 + 1], a[W4];
#pragma unroll
                    for (int j = 0; j <= W4; ++j) v[j] = wp[wr * S4 + j];
#pragma unroll
                    for (int j = 0; j < W4; ++j) a[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], shift) & cm[j];
#pragma unroll
                    for (int k = 0; k < kDy; ++k) {
                        const int r = wr - k;
                        if (r >= 0 && r < B && r < nrows) {
#pragma unroll
                            for (int j = 0; j < W4; ++j) acc[k] = __builtin_amdgcn_sad_u8(a[j], c[r < 0 || r >= B ? 0 : r][j], acc[k]);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kDy; ++k) {
                const int dyi = kDy * g + k;
                if (live && dyi < n) {
                    const int dy = dyi - R, dx = dxi - R;
                    const uint32_t cost = acc[k] + (uint32_t)(lam * (abs(dy) + abs(dx)));
                    const unsigned long long key = ((unsigned long long)cost << 26) | ((unsigned long long)(dy * dy + dx * dx) << 14) |
                                                   ((unsigned long long)(dy + kMaxR) << 7) | (unsigned long long)(dx + kMaxR);
                    best = key < best ? key : best;
                    if (dy == 0 && dx == 0) sad0[cell] = acc[k];
                }
            }
        }
        best = wave_reduce(best, WaveMinU64{});
        if (lane == 0) {
            const int dy = (int)((best >> 7) & 127) - kMaxR, dx = (int)(best & 127) - kMaxR;
            mv[cell] = ((uint32_t)dy & 0xFFFFu) | ((uint32_t)dx << 16);          // int16 (dy, dx)
            sad[cell] = (uint32_t)(best >> 26) - (uint32_t)(lam * (abs(dy) + abs(dx)));
        }
    }
}

inline bool shape_ok(int T, int H, int W) {                // the shapes hv_content_histograms takes
    return T >= 1 && T <= kMaxT && H >= 1 && W >= 1 && H <= (1 << 16) && W <= (1 << 16) && (int64_t)H * W <= 0x7fffffff;
}

template <typename T>
int launch(const void* x, int64_t sc, int64_t st, int64_t sh, int Tn, int H, int W, int rescale, Luma lu, int block, int radius, int lam,
           uint32_t* mv, uint32_t* sad, uint32_t* sad0, hipStream_t stream) {
    const int Hb = (H + block - 1) / block, Wb = (W + block - 1) / block;
    const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile), (unsigned)(Tn - 1));
    if (block == 8)
        block_motion_kernel<T, 8><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, H, W, Hb, Wb, rescale, lu, radius, lam, mv, sad, sad0);
    else
        block_motion_kernel<T, 16><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, H, W, Hb, Wb, rescale, lu, radius, lam, mv, sad, sad0);
    return hv_check_launch();
}

}  // namespace

extern "C" int hv_block_motion(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int T, int H, int W, int rescale, int wr, int wg,
                               int wb, int round, int shift, int block, int radius, int lam, void* mv, void* sad, void* sad0,
                               hipStream_t stream) {
    if (!x || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1) || !shape_ok(T, H, W)) return HV_ERR_ARG;
    // rows are W contiguous elements; rows, frames and channels may be strided (views), never overlapping backwards
    if (sh < W || sc < 0 || st < 0) return HV_ERR_ARG;
    // the luma stays a byte and its int32 arithmetic cannot overflow
    if (wr < 0 || wg < 0 || wb < 0 || round < 0 || shift < 0 || shift > 22 || wr > (1 << 22) || wg > (1 << 22) || wb > (1 << 22) ||
        ((int64_t)wr + wg + wb) * 255 + round >= ((int64_t)256 << shift))
        return HV_ERR_ARG;
    if ((block != 8 && block != 16) || radius < 1 || radius > kMaxR || lam < 0 || lam > kMaxLam) return HV_ERR_ARG;
    if (((uintptr_t)mv & 3) != 0 || ((uintptr_t)sad & 3) != 0 || ((uintptr_t)sad0 & 3) != 0) return HV_ERR_ARG;
    if (T == 1) return HV_OK;                              // no pairs: nothing to write
    if (!mv || !sad || !sad0) return HV_ERR_ARG;
    const Luma lu{wr, wg, wb, round, shift};
    if (dtype == 0)
        return launch<_Float16>(x, sc, st, sh, T, H, W, rescale, lu, block, radius, lam, (uint32_t*)mv, (uint32_t*)sad, (uint32_t*)sad0, stream);
    return launch<float>(x, sc, st, sh, T, H, W, rescale, lu, block, radius, lam, (uint32_t*)mv, (uint32_t*)sad, (uint32_t*)sad0, stream);
}
