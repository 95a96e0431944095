// Gaussian-window SSIM of two videos on the device (include/hv_gssim.h): the score of the fork's rebuttal/common_metrics_on_video_quality
// (pytorch_msssim.ssim on [B,C,T,H,W]: an 11-tap separable window over T, H and W; calculate_ssim.py: the same window per frame).  Five
// fields (x, y, xx, yy, xy) are filtered along up to three axes in fp64 - 165 multiply-adds a map position - and never reach HBM.
//
//   gssim_kernel<T, TEMPORAL>  a workgroup owns a tile of 16 x 32 map positions of one channel, i.e. a halo of 26 x 42 pixels, and walks
//                              a run of output frames.
//                              T pass (TEMPORAL): a thread keeps the last 11 frames of its (up to 5) halo pixels in registers as byte pairs
//                              (quantise() of hv_common.hpp on both videos: 11 dwords a pixel instead of 55 doubles an output).  The ring
//                              index is a compile-time constant: the frame loop dispatches on (frame mod 11) to one of 11 instantiations,
//                              so the ring stays in VGPRs.  Per output frame a new frame is loaded into the oldest place and the five
//                              11-term chains are evaluated in frame order; the results go to LDS [5][26][42].
//                              H pass: thread (field, column) slides down its column: 26 LDS reads feed 16 chains (176 fma), which keeps
//                              the pass on the fp64 pipe and off the LDS port (one read per fma would be LDS-bound four times over).
//                              W pass: thread (field, row, half) does the same along its row, rows 43 doubles apart (conflict-free).
//                              Map: the five filtered values of a position meet again through LDS; a thread evaluates two positions;
//                              wave butterfly, four waves in order, one partial per (tile, frame, channel) to the workspace.
//   gssim_fold                 adds the tiles of each [To][C] cell in tile order.  No atomics anywhere: two runs give the same bits.
#include "hv_common.hpp"
#include "../../include/hv_gssim.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kWin = HV_GSSIM_WIN, kHalo = kWin - 1;
constexpr int kTH = HV_GSSIM_TILE_H, kTW = HV_GSSIM_TILE_W;
constexpr int kHH = kTH + kHalo, kHW = kTW + kHalo;        // halo tile 26 x 42
constexpr int kHaloPx = kHH * kHW;
constexpr int kSlots = (kHaloPx + kThreads - 1) / kThreads;  // halo pixels of one thread
constexpr int kFields = 5;
constexpr int kGRow = kHW + 1, kG = kFields * kTH * kGRow;   // H-pass results [5][16][43]
constexpr int kMRow = kTW + 1, kM = kFields * kTH * kMRow;   // W-pass results [5][16][33]
constexpr int kLds = (kG + kM > kFields * kHaloPx) ? kG + kM : kFields * kHaloPx;
constexpr int kOut = kTH * kTW, kOSlots = kOut / kThreads;
static_assert(kOSlots * kThreads == kOut, "whole map positions per thread");
static_assert(kFields * kHW <= kThreads && kFields * kTH * 2 <= kThreads && kTW == 32, "one H-pass column / W-pass half row per thread");
static_assert(kLds * 8 <= 64 * 1024, "static LDS");
constexpr int kMaxT = 65535, kMaxHW = 65536;
constexpr int kMinUnits = 128, kMinSeg = 4;                // (tile, channel) units from which one workgroup walks all frames; shortest run
constexpr double kC1 = (0.01 * 255.0) * (0.01 * 255.0), kC2 = (0.03 * 255.0) * (0.03 * 255.0);

struct Strides {
    int64_t sc, st, sh;
};

template <typename T>
__device__ __forceinline__ uint32_t load_pair(const T* __restrict__ a, const T* __restrict__ b, int64_t oa, int64_t ob, int rescale) {
    if (oa < 0) return 0u;                                  // outside the frame: feeds masked map positions only
    return quantise((float)a[oa], rescale) | (quantise((float)b[ob], rescale) << 8);
}

// the five fields of a byte pair; products of bytes are exact in fp32
struct Fields {
    double v[kFields];
};
__device__ __forceinline__ Fields fields_of(uint32_t pair) {
    const float x = (float)(pair & 255u), y = (float)(pair >> 8);
    return Fields{{(double)x, (double)y, (double)(x * x), (double)(y * y), (double)(x * y)}};
}

// T pass of output frame n (n mod 11 == P) for every halo pixel of the thread: frame n + k sits at ring[(P + k) % 11]
template <int P>
__device__ __forceinline__ void t_pass(const uint32_t (&ring)[kSlots][kWin], const double (&w)[kWin], double* __restrict__ s_f, int tid) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        double acc[kFields];
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const Fields f = fields_of(ring[j][(P + k) % kWin]);
#pragma unroll
            for (int i = 0; i < kFields; ++i) acc[i] = k == 0 ? w[0] * f.v[i] : fma(w[k], f.v[i], acc[i]);
        }
        const int px = j * kThreads + tid;
        if (px < kHaloPx) {
#pragma unroll
            for (int i = 0; i < kFields; ++i) s_f[i * kHaloPx + px] = acc[i];
        }
    }
}

// NOUT consecutive outputs of a 1-D pass from NOUT + 10 inputs `stride` apart: every input is read once; output r's chain takes its
// terms k = 0 .. 10 in order
template <int NOUT>
__device__ __forceinline__ void slide(const double* __restrict__ src, int stride, const double (&w)[kWin], double (&acc)[NOUT]) {
#pragma unroll
    for (int i = 0; i < NOUT + kHalo; ++i) {
        const double v = src[i * stride];
#pragma unroll
        for (int r = 0; r < NOUT; ++r) {
            const int k = i - r;
            if (k == 0) acc[r] = w[0] * v;
            else if (k > 0 && k < kWin) acc[r] = fma(w[k], v, acc[r]);
        }
    }
}

// H pass, W pass, map and sum of one output frame whose T-filtered fields are in s[0 .. 5 * kHaloPx); ends with the tile's sum in thread 0
__device__ __forceinline__ double spatial(double* __restrict__ s, double* __restrict__ s_red, const double (&w)[kWin], int tid, int rows,
                                          int cols) {
    __syncthreads();
    double acc[kTH];
    const bool hth = tid < kFields * kHW;
    const int hf = tid / kHW, hc = tid - hf * kHW;
    if (hth) slide<kTH>(s + hf * kHaloPx + hc, kHW, w, acc);
    __syncthreads();
    if (hth) {
#pragma unroll
        for (int r = 0; r < kTH; ++r) s[(hf * kTH + r) * kGRow + hc] = acc[r];
    }
    __syncthreads();
    const bool wth = tid < kFields * kTH * 2;
    const int half = tid & 1, wr = (tid >> 1) & (kTH - 1), wf = tid >> 5;
    if (wth) {
        slide<kTW / 2>(s + (wf * kTH + wr) * kGRow + half * (kTW / 2), 1, w, acc);
#pragma unroll
        for (int x = 0; x < kTW / 2; ++x) s[kG + (wf * kTH + wr) * kMRow + half * (kTW / 2) + x] = acc[x];
    }
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int m = 0; m < kOSlots; ++m) {
        const int o = m * kThreads + tid, r = o / kTW, x = o - r * kTW;
        const double* p = s + kG + r * kMRow + x;
        const double m1 = p[0], m2 = p[kTH * kMRow], e11 = p[2 * kTH * kMRow], e22 = p[3 * kTH * kMRow], e12 = p[4 * kTH * kMRow];
        const double m11 = __dmul_rn(m1, m1), m22 = __dmul_rn(m2, m2), m12 = __dmul_rn(m1, m2);
        const double s1 = __dsub_rn(e11, m11), s2 = __dsub_rn(e22, m22), s12 = __dsub_rn(e12, m12);
        const double lum = __ddiv_rn(__dadd_rn(__dmul_rn(2.0, m12), kC1), __dadd_rn(__dadd_rn(m11, m22), kC1));
        const double cs = __ddiv_rn(__dadd_rn(__dmul_rn(2.0, s12), kC2), __dadd_rn(__dadd_rn(s1, s2), kC2));
        const double v = __dmul_rn(lum, cs);
        if (r < rows && x < cols) sum = __dadd_rn(sum, v);
    }
    sum = wave_sum(sum);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();                                        // also: every read of s is done before the next frame's T pass writes it
    return tid == 0 ? __dadd_rn(__dadd_rn(__dadd_rn(s_red[0], s_red[1]), s_red[2]), s_red[3]) : 0.0;
}

template <typename T, int P>
__device__ __forceinline__ void t_step(uint32_t (&ring)[kSlots][kWin], const T* __restrict__ a, const T* __restrict__ b,
                                       const int64_t (&oa)[kSlots], const int64_t (&ob)[kSlots], int rescale, const double (&w)[kWin],
                                       double* __restrict__ s_f, int tid) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) ring[j][(P + kHalo) % kWin] = load_pair(a, b, oa[j], ob[j], rescale);
    t_pass<P>(ring, w, s_f, tid);
}

template <typename T, bool TEMPORAL>
__global__ __launch_bounds__(kThreads) void gssim_kernel(const T* __restrict__ a, const T* __restrict__ b, Strides sa, Strides sb, int To,
                                                         int H, int W, int rescale, const double* __restrict__ win, int nseg, int seg_len,
                                                         int C, double* __restrict__ part) {
    __shared__ double s[kLds];
    __shared__ double s_red[kWaves];
    const int tid = threadIdx.x;
    const int c = blockIdx.z / nseg, seg = blockIdx.z - c * nseg;
    const int t0 = seg * seg_len, t1 = min(t0 + seg_len, To);
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const int rows = min(kTH, H - kHalo - y0), cols = min(kTW, W - kHalo - x0);   // live map positions of the tile
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    double w[kWin];
#pragma unroll
    for (int k = 0; k < kWin; ++k) w[k] = win[k];
    int64_t oa[kSlots], ob[kSlots];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
        const int px = j * kThreads + tid, hy = px / kHW, hx = px - hy * kHW;
        const bool in = px < kHaloPx && y0 + hy < H && x0 + hx < W;
        oa[j] = in ? (int64_t)(y0 + hy) * sa.sh + (x0 + hx) : -1;
        ob[j] = in ? (int64_t)(y0 + hy) * sb.sh + (x0 + hx) : -1;
    }
    a += (int64_t)c * sa.sc;
    b += (int64_t)c * sb.sc;
    double* dst = part + (tile * To) * C + c;

    if constexpr (TEMPORAL) {
        uint32_t ring[kSlots][kWin];
#pragma unroll
        for (int i = 0; i < kHalo; ++i) {                   // frames t0 .. t0 + 9 (t0 + 9 <= To + 8 = T - 2)
#pragma unroll
            for (int j = 0; j < kSlots; ++j)
                ring[j][i] = load_pair(a + (int64_t)(t0 + i) * sa.st, b + (int64_t)(t0 + i) * sb.st, oa[j], ob[j], rescale);
        }
#pragma unroll
        for (int j = 0; j < kSlots; ++j) ring[j][kHalo] = 0u;
        int phase = 0;
        for (int t = t0; t < t1; ++t) {
            const T* an = a + (int64_t)(t + kHalo) * sa.st;   // t + 10 <= To + 9 = T - 1
            const T* bn = b + (int64_t)(t + kHalo) * sb.st;
            switch (phase) {
#define HV_GSSIM_PHASE(P) case P: t_step<T, P>(ring, an, bn, oa, ob, rescale, w, s, tid); break;
                HV_GSSIM_PHASE(0) HV_GSSIM_PHASE(1) HV_GSSIM_PHASE(2) HV_GSSIM_PHASE(3) HV_GSSIM_PHASE(4) HV_GSSIM_PHASE(5)
                HV_GSSIM_PHASE(6) HV_GSSIM_PHASE(7) HV_GSSIM_PHASE(8) HV_GSSIM_PHASE(9) HV_GSSIM_PHASE(10)
#undef HV_GSSIM_PHASE
            }
            phase = phase == kWin - 1 ? 0 : phase + 1;
            const double sum = spatial(s, s_red, w, tid, rows, cols);
            if (tid == 0) dst[(int64_t)t * C] = sum;
        }
    } else {
        for (int t = t0; t < t1; ++t) {
            const T* at = a + (int64_t)t * sa.st;
            const T* bt = b + (int64_t)t * sb.st;
#pragma unroll
            for (int j = 0; j < kSlots; ++j) {
                const int px = j * kThreads + tid;
                const Fields f = fields_of(load_pair(at, bt, oa[j], ob[j], rescale));
                if (px < kHaloPx) {
#pragma unroll
                    for (int i = 0; i < kFields; ++i) s[i * kHaloPx + px] = f.v[i];
                }
            }
            const double sum = spatial(s, s_red, w, tid, rows, cols);
            if (tid == 0) dst[(int64_t)t * C] = sum;
        }
    }
}

// one thread per [To][C] cell: the tiles in order
__global__ __launch_bounds__(kThreads) void gssim_fold(const double* __restrict__ part, int64_t ntiles, int64_t cells,
                                                      double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= cells) return;
    double sum = part[idx];
    for (int64_t i = 1; i < ntiles; ++i) sum = __dadd_rn(sum, part[i * cells + idx]);
    out[idx] = sum;
}

struct Plan {
    int tx, ty, To, nseg, seg_len;
    int64_t ntiles, cells, ws_bytes;
};
inline bool plan(int C, int T, int H, int W, int temporal, Plan& p) {
    if ((C != 1 && C != 3) || T < 1 || T > kMaxT || H < kWin || W < kWin || H > kMaxHW || W > kMaxHW || (temporal != 0 && temporal != 1) ||
        (temporal == 1 && T < kWin))
        return false;
    p.To = temporal ? T - kHalo : T;
    p.tx = (W - kHalo + kTW - 1) / kTW;
    p.ty = (H - kHalo + kTH - 1) / kTH;
    p.ntiles = (int64_t)p.tx * p.ty;
    p.cells = (int64_t)p.To * C;
    p.ws_bytes = p.ntiles * p.cells * 8;
    // small frames: split the walk so that the card has workgroups (a run re-reads 10 frames, it recomputes nothing)
    const int64_t units = p.ntiles * C;
    int64_t nseg = units >= kMinUnits ? 1 : (kMinUnits + units - 1) / units;
    const int64_t most = (p.To + kMinSeg - 1) / kMinSeg;
    if (nseg > most) nseg = most;
    p.seg_len = (int)((p.To + nseg - 1) / nseg);
    p.nseg = (p.To + p.seg_len - 1) / p.seg_len;
    return true;
}

template <typename T>
int launch(const void* a, Strides sa, const void* b, Strides sb, int C, int H, int W, int rescale, int temporal, const double* win,
           double* out, double* ws, const Plan& p, hipStream_t stream) {
    const dim3 grid((unsigned)p.tx, (unsigned)p.ty, (unsigned)(C * p.nseg));
    if (temporal)
        gssim_kernel<T, true><<<grid, dim3(kThreads), 0, stream>>>((const T*)a, (const T*)b, sa, sb, p.To, H, W, rescale, win, p.nseg,
                                                                   p.seg_len, C, ws);
    else
        gssim_kernel<T, false><<<grid, dim3(kThreads), 0, stream>>>((const T*)a, (const T*)b, sa, sb, p.To, H, W, rescale, win, p.nseg,
                                                                    p.seg_len, C, ws);
    gssim_fold<<<dim3((unsigned)((p.cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream>>>(ws, p.ntiles, p.cells, out);
    return hv_check_launch();
}

}  // namespace

extern "C" int64_t hv_gaussian_ssim_workspace_bytes(int C, int T, int H, int W, int temporal) {
    Plan p;
    return plan(C, T, H, W, temporal, p) ? p.ws_bytes : 0;
}

extern "C" int hv_gaussian_ssim(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st,
                                int64_t b_sh, int dtype, int C, int T, int H, int W, int rescale, int temporal, const double* win,
                                double* ssim_sum, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
    Plan p;
    if (!a || !b || !win || !ssim_sum || !workspace || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1) ||
        !plan(C, T, H, W, temporal, p))
        return HV_ERR_ARG;
    // rows are W contiguous elements; rows, frames and channels may be strided (views), never overlapping backwards
    if (a_sh < W || b_sh < W || a_sc < 0 || a_st < 0 || b_sc < 0 || b_st < 0) return HV_ERR_ARG;
    if (((uintptr_t)win & 7) != 0 || ((uintptr_t)ssim_sum & 7) != 0 || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < p.ws_bytes)
        return HV_ERR_ARG;
    const Strides sa{a_sc, a_st, a_sh}, sb{b_sc, b_st, b_sh};
    if (dtype == 0) return launch<_Float16>(a, sa, b, sb, C, H, W, rescale, temporal, win, ssim_sum, (double*)workspace, p, stream);
    return launch<float>(a, sa, b, sb, C, H, W, rescale, temporal, win, ssim_sum, (double*)workspace, p, stream);
}
