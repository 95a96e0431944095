// Reconstruction scoring on the device: per-frame PSNR / SSIM statistics of two [C,T,H,W] videos (fp16 or fp32, values nominally in
// [-1, 1]) on the 8-bit frames save_videos_grid(..., rescale=True) would write - the reference's evaluation/compute_metrics.py:31-41
// minus the video codec.  Every value is quantised in registers exactly as utils/file_utils.py:frames_uint8 does on the host; no
// uint8 copy of the video reaches HBM.  All moments are exact integers; only the final SSIM map value is floating point (fp32),
// summed in fp64.  Workgroup partials go to a workspace with ordinary stores and are folded in a fixed order: no floating-point
// atomics, two calls on the same input give the same bits.
//
//   pass 1  metrics_stats_kernel   grid (chunks, T)      min / max of both frames, sum of squared differences (uint64)
//           metrics_stats_fold     grid (T)              -> sse[T], minmax[T][4]
//   pass 2  metrics_ssim_kernel    grid (tiles, C, T)    7x7 box sums from an LDS tile with a 6-pixel halo -> sum of the SSIM map
//           metrics_ssim_fold      grid (T)              -> ssim_sum[T][C]
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kStatsMaxChunks = 64;          // workgroups per frame in pass 1 (T fills the card)
constexpr int kStatsChunkElems = 16384;
constexpr int kWin = 7;                      // skimage's default window
constexpr int kHalo = kWin - 1;
constexpr int kTileW = 64;                   // window positions per tile: one wave = one row of 64 columns, so the vertical
constexpr int kTileH = 32;                   // pass reads consecutive dwords of one LDS row (conflict-free)
constexpr int kInW = kTileW + kHalo;         // 70
constexpr int kInH = kTileH + kHalo;         // 38
constexpr int kPxPitch = 72;                 // uint16 per LDS pixel row
constexpr int kRowsPerWave = kTileH / (kThreads / 64);   // 8 output rows per wave in the vertical pass

template <typename T> __device__ __forceinline__ float load1(const T* p) { return (float)*p; }

template <typename T, int VEC> struct Vec;
template <> struct Vec<_Float16, 8> { typedef __attribute__((ext_vector_type(8))) _Float16 type; };
template <> struct Vec<float, 4> { typedef __attribute__((ext_vector_type(4))) float type; };
template <> struct Vec<_Float16, 1> { typedef _Float16 type; };
template <> struct Vec<float, 1> { typedef float type; };

template <typename V, int VEC> __device__ __forceinline__ float lane_of(const V& v, int j) {
    if constexpr (VEC == 1) return (float)v;
    else return (float)v[j];
}

struct Strides {
    int64_t sc, st, sh;
};

// ---- pass 1 -----------------------------------------------------------------------------------------------------------------------
// One frame = C*H rows of W/VEC vectors; the chunks of a frame interleave over them (coalesced within a workgroup).
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void metrics_stats_kernel(const T* __restrict__ a, const T* __restrict__ b, Strides sa, Strides sb,
                                                                int C, int H, int W, int rescale, unsigned long long* __restrict__ sse_part,
                                                                int* __restrict__ mm_part) {
    typedef typename Vec<T, VEC>::type V;
    const int t = blockIdx.y, nchunk = gridDim.x, tid = threadIdx.x;
    const int wv = W / VEC;
    const int64_t items = (int64_t)C * H * wv;
    const T* fa = a + (int64_t)t * sa.st;
    const T* fb = b + (int64_t)t * sb.st;
    unsigned long long sse = 0;
    int mn1 = 255, mx1 = 0, mn2 = 255, mx2 = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < items; i += (int64_t)nchunk * kThreads) {
        const int row = (int)(i / wv), v = (int)(i - (int64_t)row * wv);
        const int c = row / H, h = row - c * H;
        const V va = *(const V*)(fa + c * sa.sc + h * sa.sh + (int64_t)v * VEC);
        const V vb = *(const V*)(fb + c * sb.sc + h * sb.sh + (int64_t)v * VEC);
        uint32_t acc = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int q1 = (int)quantise(lane_of<V, VEC>(va, j), rescale), q2 = (int)quantise(lane_of<V, VEC>(vb, j), rescale);
            const int d = q1 - q2;
            acc += (uint32_t)(d * d);
            mn1 = min(mn1, q1); mx1 = max(mx1, q1);
            mn2 = min(mn2, q2); mx2 = max(mx2, q2);
        }
        sse += acc;
    }
    sse = wave_sum(sse);
    mn1 = wave_min(mn1); mx1 = wave_max(mx1);
    mn2 = wave_min(mn2); mx2 = wave_max(mx2);
    __shared__ unsigned long long s_sse[kThreads / 64];
    __shared__ int s_mm[kThreads / 64][4];
    const int wave = tid >> 6;
    if ((tid & 63) == 0) {
        s_sse[wave] = sse;
        s_mm[wave][0] = mn1; s_mm[wave][1] = mx1; s_mm[wave][2] = mn2; s_mm[wave][3] = mx2;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kThreads / 64; ++w) {
            sse += s_sse[w];
            mn1 = min(mn1, s_mm[w][0]); mx1 = max(mx1, s_mm[w][1]);
            mn2 = min(mn2, s_mm[w][2]); mx2 = max(mx2, s_mm[w][3]);
        }
        const int64_t slot = (int64_t)t * nchunk + blockIdx.x;
        sse_part[slot] = sse;
        mm_part[slot * 4 + 0] = mn1; mm_part[slot * 4 + 1] = mx1; mm_part[slot * 4 + 2] = mn2; mm_part[slot * 4 + 3] = mx2;
    }
}

// one wave per frame; nchunk <= 64.  Integer sums and min/max: exact in any order.
__global__ __launch_bounds__(64) void metrics_stats_fold(const unsigned long long* __restrict__ sse_part, const int* __restrict__ mm_part,
                                                        int nchunk, long long* __restrict__ sse, int* __restrict__ minmax) {
    const int t = blockIdx.x, l = threadIdx.x;
    unsigned long long s = 0;
    int mn1 = 255, mx1 = 0, mn2 = 255, mx2 = 0;
    for (int k = l; k < nchunk; k += 64) {
        const int64_t slot = (int64_t)t * nchunk + k;
        s += sse_part[slot];
        mn1 = min(mn1, mm_part[slot * 4 + 0]); mx1 = max(mx1, mm_part[slot * 4 + 1]);
        mn2 = min(mn2, mm_part[slot * 4 + 2]); mx2 = max(mx2, mm_part[slot * 4 + 3]);
    }
    s = wave_sum(s);
    mn1 = wave_min(mn1); mx1 = wave_max(mx1);
    mn2 = wave_min(mn2); mx2 = wave_max(mx2);
    if (l == 0) {
        sse[t] = (long long)s;
        minmax[t * 4 + 0] = mn1; minmax[t * 4 + 1] = mx1; minmax[t * 4 + 2] = mn2; minmax[t * 4 + 3] = mx2;
    }
}

// ---- pass 2 -----------------------------------------------------------------------------------------------------------------------
// Tile = 32 x 64 window positions of one (frame, channel); its 38 x 70 pixels of both videos are quantised into LDS as x | y << 8.
// Horizontal 7-sums of (x, y, x^2, y^2, xy) per pixel row and column go to three dword planes [38][64] (x^2 << 11 | x, y^2 << 11 | y,
// xy: 7*255 < 2^11, 7*255^2 < 2^19); the vertical pass slides a 7-row window down a column, lanes along W.
template <typename T>
__global__ __launch_bounds__(kThreads) void metrics_ssim_kernel(const T* __restrict__ a, const T* __restrict__ b, Strides sa, Strides sb,
                                                               int H, int W, int rescale, int tiles_x, const int* __restrict__ minmax,
                                                               double* __restrict__ ssim_part) {
    __shared__ uint16_t s_px[kInH][kPxPitch];
    __shared__ uint32_t s_hx[kInH][kTileW], s_hy[kInH][kTileW], s_hxy[kInH][kTileW];
    __shared__ double s_red[kThreads / 64];
    const int tile = blockIdx.x, c = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int oy = ty * kTileH, ox = tx * kTileW;
    const T* fa = a + (int64_t)t * sa.st + (int64_t)c * sa.sc;
    const T* fb = b + (int64_t)t * sb.st + (int64_t)c * sb.sc;

    for (int i = tid; i < kInH * kInW; i += kThreads) {
        const int r = i / kInW, col = i - r * kInW;
        const int gy = oy + r, gx = ox + col;
        uint32_t v = 0;
        if (gy < H && gx < W)
            v = quantise(load1(fa + (int64_t)gy * sa.sh + gx), rescale) | (quantise(load1(fb + (int64_t)gy * sb.sh + gx), rescale) << 8);
        s_px[r][col] = (uint16_t)v;
    }
    __syncthreads();

    const int col = tid & 63, wave = tid >> 6;
    for (int r = wave; r < kInH; r += kThreads / 64) {
        uint32_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const uint32_t v = s_px[r][col + k], x = v & 255u, y = v >> 8;
            sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
        s_hx[r][col] = (sxx << 11) | sx;
        s_hy[r][col] = (syy << 11) | sy;
        s_hxy[r][col] = sxy;
    }
    __syncthreads();

    // C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = max - min of the first video's frame (all channels), as the reference passes it
    const int R = minmax[t * 4 + 1] - minmax[t * 4 + 0];
    double sum = 0.0;
    if (R > 0) {
        const float Rf = (float)R;
        const float C1 = (0.01f * Rf) * (0.01f * Rf), C2 = (0.03f * Rf) * (0.03f * Rf);
        const float inv_n2 = 1.0f / 2401.0f, inv_cov = 1.0f / 2352.0f;      // 49^2; 48 * 49 (sample covariance)
        const int r0 = wave * kRowsPerWave;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < kWin - 1; ++k) {
            const uint32_t hx = s_hx[r0 + k][col], hy = s_hy[r0 + k][col];
            sx += hx & 2047u; sxx += hx >> 11; sy += hy & 2047u; syy += hy >> 11; sxy += s_hxy[r0 + k][col];
        }
        const bool col_ok = ox + col < W - kHalo;
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            {
                const uint32_t hx = s_hx[r0 + j + kWin - 1][col], hy = s_hy[r0 + j + kWin - 1][col];
                sx += hx & 2047u; sxx += hx >> 11; sy += hy & 2047u; syy += hy >> 11; sxy += s_hxy[r0 + j + kWin - 1][col];
            }
            if (col_ok && oy + r0 + j < H - kHalo) {
                // exact integers: 49*Sxx - Sx^2 <= 49^2 * 255^2 / 4 * ... < 2^31; the cancellation of the variance happens here
                const int pxy = sx * sy;
                const int vx = 49 * sxx - sx * sx, vy = 49 * syy - sy * sy, vxy = 49 * sxy - pxy;
                const float a1 = 2.0f * (float)pxy * inv_n2 + C1;
                const float b1 = (float)(sx * sx + sy * sy) * inv_n2 + C1;
                const float a2 = 2.0f * (float)vxy * inv_cov + C2;
                const float b2 = (float)(vx + vy) * inv_cov + C2;
                sum += (double)((a1 * a2) / (b1 * b2));
            }
            {
                const uint32_t hx = s_hx[r0 + j][col], hy = s_hy[r0 + j][col];
                sx -= hx & 2047u; sxx -= hx >> 11; sy -= hy & 2047u; syy -= hy >> 11; sxy -= s_hxy[r0 + j][col];
            }
        }
    }
    sum = wave_sum(sum);
    if (col == 0) s_red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double s = s_red[0];
        for (int w = 1; w < kThreads / 64; ++w) s += s_red[w];
        ssim_part[((int64_t)t * gridDim.y + c) * gridDim.x + tile] = s;
    }
}

// one wave per frame: lane l adds tiles l, l + 64, ... in order, then the butterfly: one fixed order for a given shape
__global__ __launch_bounds__(64) void metrics_ssim_fold(const double* __restrict__ ssim_part, int C, int tiles, double* __restrict__ ssim_sum) {
    const int t = blockIdx.x, l = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        const double* p = ssim_part + ((int64_t)t * C + c) * tiles;
        double s = 0.0;
        for (int k = l; k < tiles; k += 64) s += p[k];
        s = wave_sum(s);
        if (l == 0) ssim_sum[t * C + c] = s;
    }
}

inline int stats_chunks(int C, int H, int W) {
    const int64_t n = ((int64_t)C * H * W + kStatsChunkElems - 1) / kStatsChunkElems;
    return (int)(n < 1 ? 1 : n > kStatsMaxChunks ? kStatsMaxChunks : n);
}
inline int64_t ssim_tiles_x(int W) { return (W - kHalo + kTileW - 1) / kTileW; }
inline int64_t ssim_tiles_y(int H) { return (H - kHalo + kTileH - 1) / kTileH; }
inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

struct Layout {
    int nchunk;
    int64_t tiles, off_mm, off_ssim, bytes;
};
inline Layout layout(int C, int T, int H, int W) {
    Layout L;
    L.nchunk = stats_chunks(C, H, W);
    L.tiles = ssim_tiles_x(W) * ssim_tiles_y(H);
    L.off_mm = align16((int64_t)T * L.nchunk * 8);
    L.off_ssim = L.off_mm + align16((int64_t)T * L.nchunk * 16);
    L.bytes = L.off_ssim + align16((int64_t)T * C * L.tiles * 8);
    return L;
}
inline bool shape_ok(int C, int T, int H, int W) {
    return (C == 1 || C == 3) && T >= 1 && T <= 65535 && H >= kWin && W >= kWin && H <= (1 << 16) && W <= (1 << 16);
}

template <typename T>
int launch(const T* a, const T* b, Strides sa, Strides sb, int C, int Tn, int H, int W, int rescale, int passes, long long* sse, int* minmax,
           double* ssim_sum, char* ws, const Layout& L, hipStream_t stream) {
    unsigned long long* sse_part = (unsigned long long*)ws;
    int* mm_part = (int*)(ws + L.off_mm);
    double* ssim_part = (double*)(ws + L.off_ssim);
    constexpr int VEC = sizeof(T) == 2 ? 8 : 4;
    auto vec_ok = [&](const T* p, const Strides& s) {
        return ((uintptr_t)p & 15) == 0 && s.sc % VEC == 0 && s.st % VEC == 0 && s.sh % VEC == 0;
    };
    const dim3 g1(L.nchunk, Tn);
    if (passes & 1) {
        if (W % VEC == 0 && vec_ok(a, sa) && vec_ok(b, sb))
            metrics_stats_kernel<T, VEC><<<g1, dim3(kThreads), 0, stream>>>(a, b, sa, sb, C, H, W, rescale, sse_part, mm_part);
        else
            metrics_stats_kernel<T, 1><<<g1, dim3(kThreads), 0, stream>>>(a, b, sa, sb, C, H, W, rescale, sse_part, mm_part);
        metrics_stats_fold<<<dim3(Tn), dim3(64), 0, stream>>>(sse_part, mm_part, L.nchunk, sse, minmax);
    }
    if (!(passes & 2)) return hv_check_launch();
    metrics_ssim_kernel<T><<<dim3((unsigned)L.tiles, C, Tn), dim3(kThreads), 0, stream>>>(a, b, sa, sb, H, W, rescale, (int)ssim_tiles_x(W),
                                                                                        minmax, ssim_part);
    metrics_ssim_fold<<<dim3(Tn), dim3(64), 0, stream>>>(ssim_part, C, (int)L.tiles, ssim_sum);
    return hv_check_launch();
}

}  // namespace

extern "C" int64_t hv_video_metrics_workspace_bytes(int C, int T, int H, int W) {
    if (!shape_ok(C, T, H, W)) return 0;
    return layout(C, T, H, W).bytes;
}

extern "C" int hv_video_metrics(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st,
                                int64_t b_sh, int dtype, int C, int T, int H, int W, int rescale, int passes, void* sse, void* minmax,
                                void* ssim_sum, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
    if (!a || !b || !sse || !minmax || !ssim_sum || !workspace || !shape_ok(C, T, H, W) || (dtype != 0 && dtype != 1) ||
        (rescale != 0 && rescale != 1) || passes < 1 || passes > 3)
        return HV_ERR_ARG;
    // rows are W contiguous elements; rows, frames and channels may be strided (views), never overlapping backwards
    if (a_sh < W || b_sh < W || a_sc < 0 || a_st < 0 || b_sc < 0 || b_st < 0) return HV_ERR_ARG;
    if (((uintptr_t)workspace & 15) != 0) return HV_ERR_ARG;
    const Layout L = layout(C, T, H, W);
    if (workspace_bytes < L.bytes) return HV_ERR_ARG;
    const Strides sa{a_sc, a_st, a_sh}, sb{b_sc, b_st, b_sh};
    if (dtype == 0)
        return launch<_Float16>((const _Float16*)a, (const _Float16*)b, sa, sb, C, T, H, W, rescale, passes, (long long*)sse, (int*)minmax,
                                (double*)ssim_sum, (char*)workspace, L, stream);
    return launch<float>((const float*)a, (const float*)b, sa, sb, C, T, H, W, rescale, passes, (long long*)sse, (int*)minmax, (double*)ssim_sum,
                         (char*)workspace, L, stream);
}
