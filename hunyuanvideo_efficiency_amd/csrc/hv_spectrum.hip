// Temporal spectra on the device: the fork's theory_analysis.ipynb cells 2, 4 and 5 - np.abs(np.fft.fft(signal, axis=0)).mean(axis=1) over
// every pixel time series of the 8-bit gray frames of a clip, and over every (channel, h, w) series of latent_dist.mean - as per-bin
// sums of |X_k| and |X_k|^2 over all series of one [C,T,H,W] tensor (fp16 or fp32, element strides, W contiguous: hv_metrics.hip's
// conventions).  The transform never reaches HBM.
//
//   spectrum_kernel<T, GRAY>   one series per thread: GRAY quantises R, G, B to the bytes frames_uint8 would write (quantise(),
//                              hv_common.hpp) and forms the integer luma (wr R + wg G + wb B + round) >> shift; otherwise the value is
//                              cast to fp32.  d_t = x_t - x_0 (exact for the integers, one fp32 rounding otherwise): X_k(d) = X_k(x)
//                              for k >= 1, and a near-static series keeps its small motion instead of losing it to the cancellation
//                              of a large DC term.  Bin 0 is sum_t x_t itself (exact integers, or an fp32 chain in frame order).
//                              re_k, im_k = sum_t d_t cos / sin(2 pi (k t mod T) / T), k = 1 .. T/2: an fp32 GEMM [series, T] x [T, 2 T/2]
//                              on v_mfma_f32_32x32x2_f32 against the host's twiddle table (float64 entries of the integer-reduced
//                              angle, rounded once; rows behind T zero).
//   spectrum_fold              one wave per bin adds the workgroup partials in a fixed order -> mag_sum[K], pow_sum[K]
//
// Block tile 256 series x 64 columns x 32 frames, as lpips_conv_kernel (hv_lpips.hip): k-major LDS tiles, so the 32 lanes that share a
// frame read 32 consecutive dwords, and the next 32 frames are fetched into registers while the MFMAs of this chunk run.  A column tile
// is the cos block of 32 bins followed by the sin block of the same bins; a wave owns 64 series x both blocks, so re_k and im_k of one
// (series, k) are the same register of two accumulators of one lane and |X_k|^2 = re^2 + im^2 needs no shuffle.  Each thread keeps
// fp64 sums over its rows and over the row tiles its workgroup walks (at most 1024 row workgroups, then a second trip); they meet once,
// in a fixed order, at the end: no atomics, two calls give the same bits.  Rows behind the series count hold d = 0 and add nothing.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int BM = 256, BN = 64, BK = HV_SPECTRUM_BK;
constexpr int kBins = HV_SPECTRUM_BINS;      // bins per column tile
static_assert(kBins == BN / 2, "a column tile is the cos block and the sin block of the same bins");
constexpr int kMaxT = HV_SPECTRUM_MAX_T;
constexpr int kMaxRowWgs = 1024;             // row workgroups of a launch; row tile g + i * 1024 is trip i of workgroup g

struct Luma {
    int wr, wg, wb, round, shift;
};

template <typename T, bool GRAY>
__global__ __launch_bounds__(kThreads) void spectrum_kernel(const T* __restrict__ x, int64_t sc, int64_t st, int64_t sh, int Tn, int HW, int W,
                                                           int64_t N, int rescale, Luma lu, const float* __restrict__ tw, int ncol, int nk,
                                                           int64_t mtiles, int nrow, double* __restrict__ part_mag,
                                                           double* __restrict__ part_pow) {
    __shared__ float sA[BK * BM];
    __shared__ __attribute__((aligned(16))) float sB[BK * BN];
    __shared__ double s_red[kThreads / 64][kBins][2];
    __shared__ double s_dc[kThreads / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x / ncol, ct = blockIdx.x - g * ncol;  // the column tiles of one row tile are neighbours in the grid
    const int ldt = ncol * BN;
    constexpr int NC = GRAY ? 3 : 1;

    const int bk = tid >> 4, bn = (tid & 15) * 4;                 // B: rows bk and bk + 16 of the chunk, 4 columns
    const float* wp = tw + (int64_t)bk * ldt + ct * BN + bn;
    f32x4 vb0, vb1;
    auto fetch_b = [&](int kc) {
        const float* p = wp + (int64_t)kc * BK * ldt;
        vb0 = *(const f32x4*)p;
        vb1 = *(const f32x4*)(p + (int64_t)16 * ldt);
    };

    const int wm = wave * 64;
    const int lr = lane & 31, lk = lane >> 5;
    double mag_acc = 0.0, pow_acc = 0.0;     // column lr of this wave: its rows, every trip
    double dc_mag = 0.0, dc_pow = 0.0;       // this thread's series, every trip

    for (int64_t mt = g; mt < mtiles; mt += nrow) {
        const int64_t m = mt * BM + tid;
        const bool ok = m < N;
        const T* base = x;
        if (ok) {
            if constexpr (GRAY) {
                const int h = (int)(m / W);
                base = x + h * sh + (m - (int64_t)h * W);
            } else {
                const int c = (int)(m / HW), r = (int)(m - (int64_t)c * HW);
                const int h = r / W;
                base = x + c * sc + h * sh + (r - h * W);
            }
        }
        auto value = [&](const T (&v)[NC]) -> float {             // the series' sample, an integer in gray mode
            if constexpr (GRAY) {
                const int y = (lu.wr * (int)quantise((float)v[0], rescale) + lu.wg * (int)quantise((float)v[1], rescale) +
                               lu.wb * (int)quantise((float)v[2], rescale) + lu.round) >> lu.shift;
                return (float)y;
            } else {
                return (float)v[0];
            }
        };
        T raw[BK][NC];
        auto fetch_a = [&](int kc) {
#pragma unroll
            for (int j = 0; j < BK; ++j) {
                const int t = kc * BK + j;
#pragma unroll
                for (int c = 0; c < NC; ++c) raw[j][c] = ok && t < Tn ? base[t * st + c * sc] : (T)0;
            }
        };
        float x0 = 0.f;
        if (ok) {
            T v0[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) v0[c] = base[c * sc];
            x0 = value(v0);
        }
        float dc = 0.f;                      // gray: integers below 2^24, exact in fp32 (255 * 1024 < 2^18)
        f32x16 re0 = {}, im0 = {}, re1 = {}, im1 = {};
        fetch_a(0);
        fetch_b(0);
        for (int kc = 0; kc < nk; ++kc) {
#pragma unroll
            for (int j = 0; j < BK; ++j) {
                float d = 0.f;
                if (ok && kc * BK + j < Tn) {
                    const float v = value(raw[j]);
                    dc = __fadd_rn(dc, v);
                    d = __fsub_rn(v, x0);
                }
                sA[j * BM + tid] = d;
            }
            *(f32x4*)(sB + bk * BN + bn) = vb0;
            *(f32x4*)(sB + (bk + 16) * BN + bn) = vb1;
            __syncthreads();
            if (kc + 1 < nk) {
                fetch_a(kc + 1);
                fetch_b(kc + 1);
            }
#pragma unroll
            for (int ks = 0; ks < BK / 2; ++ks) {
                const int k = ks * 2 + lk;
                const float a0 = sA[k * BM + wm + lr], a1 = sA[k * BM + wm + 32 + lr];
                const float bc = sB[k * BN + lr], bs = sB[k * BN + kBins + lr];
                re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bc, re0, 0, 0, 0);
                im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bs, im0, 0, 0, 0);
                re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bc, re1, 0, 0, 0);
                im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bs, im1, 0, 0, 0);
            }
            __syncthreads();
        }
        // C/D map of the 32x32 forms: column = lane & 31 (the bin), rows in the registers: a plain sum over them
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p0 = __fadd_rn(__fmul_rn(re0[r], re0[r]), __fmul_rn(im0[r], im0[r]));
            const float p1 = __fadd_rn(__fmul_rn(re1[r], re1[r]), __fmul_rn(im1[r], im1[r]));
            mag_acc += (double)__fsqrt_rn(p0);
            pow_acc += (double)p0;
            mag_acc += (double)__fsqrt_rn(p1);
            pow_acc += (double)p1;
        }
        dc_mag += (double)fabsf(dc);
        if constexpr (GRAY) dc_pow += (double)dc * (double)dc;    // exact: an integer below 2^36
        else dc_pow += (double)__fmul_rn(dc, dc);
    }

    mag_acc += __shfl_xor(mag_acc, 32, 64);
    pow_acc += __shfl_xor(pow_acc, 32, 64);
    if (lk == 0) {
        s_red[wave][lr][0] = mag_acc;
        s_red[wave][lr][1] = pow_acc;
    }
    if (ct == 0) {
        dc_mag = wave_sum(dc_mag);
        dc_pow = wave_sum(dc_pow);
        if (lane == 0) {
            s_dc[wave][0] = dc_mag;
            s_dc[wave][1] = dc_pow;
        }
    }
    __syncthreads();
    if (tid < kBins) {
        const int bin = 1 + ct * kBins + tid;
        if (bin <= Tn / 2) {
            double sm = s_red[0][tid][0], sp = s_red[0][tid][1];
            for (int wv = 1; wv < kThreads / 64; ++wv) {
                sm += s_red[wv][tid][0];
                sp += s_red[wv][tid][1];
            }
            part_mag[(int64_t)bin * nrow + g] = sm;
            part_pow[(int64_t)bin * nrow + g] = sp;
        }
    } else if (tid == 64 && ct == 0) {
        double sm = s_dc[0][0], sp = s_dc[0][1];
        for (int wv = 1; wv < kThreads / 64; ++wv) {
            sm += s_dc[wv][0];
            sp += s_dc[wv][1];
        }
        part_mag[g] = sm;
        part_pow[g] = sp;
    }
}

// one wave per bin: lane l adds partials l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void spectrum_fold(const double* __restrict__ part_mag, const double* __restrict__ part_pow, int nrow,
                                                   double* __restrict__ mag_sum, double* __restrict__ pow_sum) {
    const int k = blockIdx.x, l = threadIdx.x;
    double sm = 0.0, sp = 0.0;
    for (int i = l; i < nrow; i += 64) {
        sm += part_mag[(int64_t)k * nrow + i];
        sp += part_pow[(int64_t)k * nrow + i];
    }
    sm = wave_sum(sm);
    sp = wave_sum(sp);
    if (l == 0) {
        mag_sum[k] = sm;
        pow_sum[k] = sp;
    }
}

struct Plan {
    int64_t N, mtiles, ws_bytes, tw_floats;
    int nrow, ncol, nk, K;
};
inline bool plan(int mode, int C, int T, int H, int W, Plan& p) {
    if ((mode != 0 && mode != 1) || T < 1 || T > kMaxT || C < 1 || C > (1 << 16) || H < 1 || W < 1 || H > (1 << 16) || W > (1 << 16))
        return false;
    if (mode == 0 && C != 3) return false;
    if ((int64_t)H * W > 0x7fffffff) return false;
    p.N = (int64_t)(mode == 0 ? 1 : C) * H * W;
    p.mtiles = (p.N + BM - 1) / BM;
    p.nrow = (int)(p.mtiles < kMaxRowWgs ? p.mtiles : kMaxRowWgs);
    p.K = T / 2 + 1;
    p.ncol = p.K - 1 < 1 ? 1 : (p.K - 1 + kBins - 1) / kBins;
    p.nk = (T + BK - 1) / BK;
    p.ws_bytes = (int64_t)2 * p.K * p.nrow * 8;
    p.tw_floats = (int64_t)p.nk * BK * p.ncol * BN;
    return true;
}

template <typename T>
int launch(const void* x, int64_t sc, int64_t st, int64_t sh, int mode, int Tn, int H, int W, int rescale, Luma lu, const float* tw,
           double* mag_sum, double* pow_sum, double* ws, const Plan& p, hipStream_t stream) {
    double* part_mag = ws;
    double* part_pow = ws + (int64_t)p.K * p.nrow;
    const dim3 grid((unsigned)(p.nrow * p.ncol));
    if (mode == 0)
        spectrum_kernel<T, true><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, Tn, H * W, W, p.N, rescale, lu, tw, p.ncol, p.nk,
                                                                      p.mtiles, p.nrow, part_mag, part_pow);
    else
        spectrum_kernel<T, false><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, Tn, H * W, W, p.N, rescale, lu, tw, p.ncol,
                                                                       p.nk, p.mtiles, p.nrow, part_mag, part_pow);
    spectrum_fold<<<dim3(p.K), dim3(64), 0, stream>>>(part_mag, part_pow, p.nrow, mag_sum, pow_sum);
    return hv_check_launch();
}

}  // namespace

extern "C" int64_t hv_temporal_spectrum_workspace_bytes(int mode, int C, int T, int H, int W) {
    Plan p;
    return plan(mode, C, T, H, W, p) ? p.ws_bytes : 0;
}

extern "C" int hv_temporal_spectrum(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int mode, int C, int T, int H, int W,
                                    int rescale, int wr, int wg, int wb, int round, int shift, const float* twiddle, int64_t twiddle_floats,
                                    double* mag_sum, double* pow_sum, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
    Plan p;
    if (!x || !twiddle || !mag_sum || !pow_sum || !workspace || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1) ||
        !plan(mode, C, T, H, W, p))
        return HV_ERR_ARG;
    // rows are W contiguous elements; rows, frames and channels may be strided (views), never overlapping backwards
    if (sh < W || sc < 0 || st < 0) return HV_ERR_ARG;
    if (mode == 0) {
        // the luma stays a byte and its int32 arithmetic cannot overflow
        if (wr < 0 || wg < 0 || wb < 0 || round < 0 || shift < 0 || shift > 22 || wr > (1 << 22) || wg > (1 << 22) || wb > (1 << 22) ||
            ((int64_t)wr + wg + wb) * 255 + round >= ((int64_t)256 << shift))
            return HV_ERR_ARG;
    }
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)twiddle & 15) != 0 || workspace_bytes < p.ws_bytes || twiddle_floats < p.tw_floats)
        return HV_ERR_ARG;
    const Luma lu{wr, wg, wb, round, shift};
    if (dtype == 0)
        return launch<_Float16>(x, sc, st, sh, mode, T, H, W, rescale, lu, twiddle, mag_sum, pow_sum, (double*)workspace, p, stream);
    return launch<float>(x, sc, st, sh, mode, T, H, W, rescale, lu, twiddle, mag_sum, pow_sum, (double*)workspace, p, stream);
}
