// Inception-I3D logits for the Frechet Video Distance (the fork's rebuttal/common_metrics_on_video_quality/calculate_fvd.py with
// method='videogpt': fvd/videogpt/pytorch_i3d.py is the network, fvd/videogpt/fvd.py:21-60 the preprocessing), in fp32 like the reference.
//
//   i3d_preprocess_kernel<T>   [3,T,H,W] fp16 / fp32 video -> [T,224,224,4] fp32: 8-bit quantisation in registers (frames_uint8, as
//                              hv_metrics.hip), b / 255, bilinear resize (align_corners=False) of the shorter side to 224, centre crop,
//                              (v - 0.5) * 2; channel 3 = 0
//   i3d_conv_kernel            Unit3D: zero-padded 3-D convolution (extents 1 | 3 | 7, strides 1 | 2) + folded BatchNorm (or bias) +
//                              optional ReLU, as an implicit GEMM on the fp32-input MFMA block tile of hv_common.hpp (f32tile)
//   i3d_maxpool_kernel         MaxPool3dSamePadding: zero padding that takes part in the maximum; a NaN cell gives a NaN
//   i3d_head_pool / _logits    AvgPool3d([2,7,7]) + the 1024 -> 400 logits layer + the mean over time
//
// Features are channels-last fp32 [voxel = (t * H + h) * W + w][C] with a row pitch: every kernel reads a column slice of a wider
// buffer and writes one, so the branches of an Inception module land in their slice of the module's output (no concatenation).
// Element offsets are 64-bit.  k of the implicit GEMM = ((dt * kh + dh) * kw + dw) * Cin + ci; Cin % 4 == 0 keeps a thread's four
// consecutive k inside one tap (one 16-byte load); a k-chunk of 32 may span several taps, so each thread decodes its own.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"

namespace {

using namespace f32tile;

struct ConvGeom {
    int H, W, T;                             // input extents
    int OH, OW;                              // output extents (OT only enters through M)
    int kh, kw;                              // kernel extents (kt only enters through K)
    int st, sh, sw, pt, ph, pw;
    int Cin, K;                              // K = kt * kh * kw * Cin
};

// top-left-front input coordinate of an output row's window (t very negative: row beyond M)
struct Row3 {
    int t0, y0, x0;
};
__device__ __forceinline__ Row3 decode_row3(int64_t m, int64_t M, const ConvGeom& g) {
    Row3 r;
    if (m >= M) {
        r.t0 = -(1 << 28); r.y0 = 0; r.x0 = 0;
        return r;
    }
    const int pix = g.OH * g.OW;
    const int ot = (int)(m / pix);
    const int p = (int)(m - (int64_t)ot * pix);
    const int oy = p / g.OW;
    r.t0 = ot * g.st - g.pt;
    r.y0 = oy * g.sh - g.ph;
    r.x0 = (p - oy * g.OW) * g.sw - g.pw;
    return r;
}

// y[m][n] = act(sc[n] * sum_k A[m][k] w[k][n] + sh[n]); w is [nk * 32][Cout] (k-major, zero rows behind K).  Thread (row = tid >> 3
// (+32, +64, +96), quad = tid & 7) moves one float4 of A per row: 8 lanes read 128 bytes of consecutive k.
__global__ __launch_bounds__(kThreads) void i3d_conv_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                           const float* __restrict__ sc, const float* __restrict__ sh,
                                                           float* __restrict__ y, int64_t ldy, const ConvGeom g, int64_t M, int Cout,
                                                           int nk, int relu) {
    __shared__ float sA[BK * LDA];
    __shared__ __attribute__((aligned(16))) float sB[BK * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntn = (Cout + BN - 1) / BN;
    const int64_t m0 = (int64_t)(blockIdx.x / ntn) * BM;          // the column tiles of one row tile are neighbours in the grid
    const int n0 = (int)(blockIdx.x % ntn) * BN;

    Row3 rows[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = decode_row3(m0 + (tid >> 3) + 32 * i, M, g);
    f32x4 va[4];
    auto fetch_a = [&](int kc) {
        const int k = kc * BK + (tid & 7) * 4;
        const int tap = k / g.Cin, ci = k - tap * g.Cin;
        const int t2 = tap / g.kw, dw = tap - t2 * g.kw;
        const int dt = t2 / g.kh, dh = t2 - dt * g.kh;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int it = rows[i].t0 + dt, iy = rows[i].y0 + dh, ix = rows[i].x0 + dw;
            va[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (k < g.K && it >= 0 && it < g.T && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                va[i] = *(const f32x4*)(x + (((int64_t)it * g.H + iy) * g.W + ix) * ldx + ci);
        }
    };

    const int bk = tid >> 4, bn = (tid & 15) * 4;                 // B: rows bk and bk + 16 of the chunk, 4 columns (Cout % 4 == 0)
    const bool b_live = n0 + bn < Cout;
    const float* wp = w + (int64_t)bk * Cout + n0 + bn;
    f32x4 vb0, vb1;
    auto fetch_b = [&](int kc) {
        vb0 = vb1 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (b_live) {
            const float* p = wp + (int64_t)kc * BK * Cout;
            vb0 = *(const f32x4*)p;
            vb1 = *(const f32x4*)(p + (int64_t)16 * Cout);
        }
    };

    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 32;
    const int lr = lane & 31, lk = lane >> 5;
    f32x16 acc0 = {}, acc1 = {};
    fetch_a(0);
    fetch_b(0);
    for (int kc = 0; kc < nk; ++kc) {
        const int q = (tid & 7) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sA[(q + j) * LDA + (tid >> 3) + 32 * i] = va[i][j];
        *(f32x4*)(sB + bk * BN + bn) = vb0;
        *(f32x4*)(sB + (bk + 16) * BN + bn) = vb1;
        __syncthreads();
        if (kc + 1 < nk) {
            fetch_a(kc + 1);
            fetch_b(kc + 1);
        }
        mma_chunk(sA, sB, wm, wn, lr, lk, acc0, acc1);
        __syncthreads();
    }

    const int n = n0 + wn + lr;
    if (n >= Cout) return;
    const float scv = sc[n], shv = sh[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t ma = m0 + wm + acc_row(r, lk), mb = ma + 32;
        float ya = __fmaf_rn(acc0[r], scv, shv), yb = __fmaf_rn(acc1[r], scv, shv);
        if (relu) {
            ya = fmaxf(ya, 0.f);
            yb = fmaxf(yb, 0.f);
        }
        if (ma < M) y[ma * ldy + n] = ya;
        if (mb < M) y[mb * ldy + n] = yb;
    }
}

// ---- max pool: cells outside the input hold 0 and take part (F.pad, then MaxPool3d) ------------------------------------------------------
struct PoolGeom {
    int T, H, W, OH, OW;
    int kt, kh, kw, st, sh, sw, pt, ph, pw;
};
__global__ __launch_bounds__(kThreads) void i3d_maxpool_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                                                              const PoolGeom g, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    const int64_t m = i / C4;
    const int pix = g.OH * g.OW;
    const int ot = (int)(m / pix);
    const int p = (int)(m - (int64_t)ot * pix);
    const int oy = p / g.OW, ox = p - oy * g.OW;
    const int t0 = ot * g.st - g.pt, y0 = oy * g.sh - g.ph, x0 = ox * g.sw - g.pw;
    const float ninf = -__builtin_huge_valf();
    f32x4 best = {ninf, ninf, ninf, ninf};
    for (int dt = 0; dt < g.kt; ++dt)
        for (int dh = 0; dh < g.kh; ++dh)
            for (int dw = 0; dw < g.kw; ++dw) {
                const int it = t0 + dt, iy = y0 + dh, ix = x0 + dw;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (it >= 0 && it < g.T && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                    v = *(const f32x4*)(x + (((int64_t)it * g.H + iy) * g.W + ix) * ldx + c * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) best[j] = (v[j] > best[j] || v[j] != v[j]) ? v[j] : best[j];   // keeps a NaN, as max_pool3d does
            }
    *(f32x4*)(y + m * ldy + c * 4) = best;
}

// ---- head ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kHeadC = 1024, kHeadN = 400, kHeadHW = 49, kHeadTB = 8;

// avg[t][c] = (sum over frames t, t + 1 and their 49 voxels of x[.][c], in that order) / 98; one workgroup per t, 4 channels per thread
__global__ __launch_bounds__(kThreads) void i3d_head_pool(const float* __restrict__ x, int64_t ldx, float* __restrict__ avg) {
    const int t = blockIdx.x, c = threadIdx.x * 4;
    const float* p = x + (int64_t)t * kHeadHW * ldx + c;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < 2 * kHeadHW; ++v) {
        const f32x4 u = *(const f32x4*)(p + (int64_t)v * ldx);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = __fadd_rn(s[j], u[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = __fdiv_rn(s[j], 98.0f);
    *(f32x4*)(avg + (int64_t)t * kHeadC + c) = s;
}

// out[n] = mean over t of (bias[n] + sum_k avg[t][k] w[k][n]): one thread per n, each dot product one k-ordered fmaf chain, the mean
// summed in t order
__global__ __launch_bounds__(64) void i3d_head_logits(const float* __restrict__ avg, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out, int nt) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= kHeadN) return;
    const float bv = bias[n];
    float sum = 0.f;
    for (int t0 = 0; t0 < nt; t0 += kHeadTB) {
        float acc[kHeadTB];
#pragma unroll
        for (int j = 0; j < kHeadTB; ++j) acc[j] = 0.f;
        for (int k = 0; k < kHeadC; ++k) {
            const float wv = w[(int64_t)k * kHeadN + n];
#pragma unroll
            for (int j = 0; j < kHeadTB; ++j)
                if (t0 + j < nt) acc[j] = __fmaf_rn(avg[(int64_t)(t0 + j) * kHeadC + k], wv, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < kHeadTB; ++j)
            if (t0 + j < nt) sum = __fadd_rn(sum, __fadd_rn(acc[j], bv));
    }
    out[n] = __fdiv_rn(sum, (float)nt);
}

// ---- preprocessing ------------------------------------------------------------------------------------------------------------------------
// source coordinate of torch's bilinear resize (align_corners=False, no antialiasing) as ONE fma, which is what reproduces
// F.interpolate's coordinates: the un-fused product is up to 900 units of 2^-24 away at 1080 x 1920, the fused form under 2
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap bilinear_tap(int dst, float scale, int in) {
    const float src = fmaxf(0.0f, __fmaf_rn(scale, (float)dst + 0.5f, -0.5f));
    Tap t;
    t.i0 = min((int)src, in - 1);            // src >= 0: the cast is the floor
    t.i1 = min(t.i0 + 1, in - 1);
    t.l1 = __fsub_rn(src, (float)t.i0);
    t.l0 = __fsub_rn(1.0f, t.l1);
    return t;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void i3d_preprocess_kernel(const T* __restrict__ x, int64_t sc, int64_t st, int64_t sh, int Tn, int H,
                                                                 int W, int RH, int RW, int rescale, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)Tn * 224 * 224) return;
    const int ox = (int)(i % 224), oy = (int)(i / 224 % 224);
    const int64_t t = i / (224 * 224);
    const Tap ty = bilinear_tap(oy + (RH - 224) / 2, (float)H / (float)RH, H);
    const Tap tx = bilinear_tap(ox + (RW - 224) / 2, (float)W / (float)RW, W);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T* p = x + c * sc + t * st;
        auto val = [&](int iy, int ix) { return __fdiv_rn((float)quantise((float)p[iy * sh + ix], rescale), 255.0f); };
        const float top = __fadd_rn(__fmul_rn(tx.l0, val(ty.i0, tx.i0)), __fmul_rn(tx.l1, val(ty.i0, tx.i1)));
        const float bot = __fadd_rn(__fmul_rn(tx.l0, val(ty.i1, tx.i0)), __fmul_rn(tx.l1, val(ty.i1, tx.i1)));
        const float v = __fadd_rn(__fmul_rn(ty.l0, top), __fmul_rn(ty.l1, bot));
        o[c] = __fmul_rn(__fsub_rn(v, 0.5f), 2.0f);
    }
    *(f32x4*)(y + i * 4) = o;
}

inline bool extent_ok(int k, int s, int p) { return (k == 1 || k == 3 || k == 7) && (s == 1 || s == 2) && p >= 0 && p < k; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int hv_i3d_conv3d_f32(const float* x, int64_t ldx, const float* w, const float* sc, const float* sh, float* y, int64_t ldy, int T,
                                 int H, int W, int Cin, int Cout, int kt, int kh, int kw, int st, int sh_, int sw, int pt, int ph, int pw,
                                 int relu, hipStream_t stream) {
    if (!x || !w || !sc || !sh || !y || (relu != 0 && relu != 1)) return HV_ERR_ARG;
    if (T < 1 || H < 1 || W < 1 || T > (1 << 16) || H > (1 << 16) || W > (1 << 16) || (int64_t)T * H * W > 0x7fffffff) return HV_ERR_ARG;
    if (Cin < 4 || Cin % 4 != 0 || Cin > 4096 || Cout < 4 || Cout % 4 != 0 || Cout > 4096) return HV_ERR_ARG;
    if (!extent_ok(kt, st, pt) || !extent_ok(kh, sh_, ph) || !extent_ok(kw, sw, pw)) return HV_ERR_ARG;
    if (ldx < Cin || ldx % 4 != 0 || ldy < Cout || !hv_aligned16(x) || !hv_aligned16(w)) return HV_ERR_ARG;
    ConvGeom g;
    g.T = T; g.H = H; g.W = W;
    const int OT = ceil_div(T, st);
    g.OH = ceil_div(H, sh_); g.OW = ceil_div(W, sw);
    g.kh = kh; g.kw = kw;
    g.st = st; g.sh = sh_; g.sw = sw; g.pt = pt; g.ph = ph; g.pw = pw;
    g.Cin = Cin; g.K = kt * kh * kw * Cin;
    const int64_t M = (int64_t)OT * g.OH * g.OW;
    const int64_t blocks = (M + BM - 1) / BM * ceil_div(Cout, BN);
    if (blocks > 0x7fffffff) return HV_ERR_ARG;
    i3d_conv_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(x, ldx, w, sc, sh, y, ldy, g, M, Cout, ceil_div(g.K, BK), relu);
    return hv_check_launch();
}

extern "C" int hv_i3d_maxpool3d_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int T, int H, int W, int C, int kt, int kh, int kw,
                                    int st, int sh_, int sw, int pt, int ph, int pw, hipStream_t stream) {
    if (!x || !y || T < 1 || H < 1 || W < 1 || T > (1 << 16) || H > (1 << 16) || W > (1 << 16) || (int64_t)T * H * W > 0x7fffffff)
        return HV_ERR_ARG;
    if (C < 4 || C % 4 != 0 || C > 4096 || ldx < C || ldx % 4 != 0 || ldy < C || ldy % 4 != 0) return HV_ERR_ARG;
    const int ks[3] = {kt, kh, kw}, ss[3] = {st, sh_, sw}, ps[3] = {pt, ph, pw};
    for (int a = 0; a < 3; ++a)
        if (ks[a] < 1 || ks[a] > 3 || ss[a] < 1 || ss[a] > 2 || ps[a] < 0 || ps[a] >= ks[a]) return HV_ERR_ARG;
    if (!hv_aligned16(x) || !hv_aligned16(y)) return HV_ERR_ARG;
    PoolGeom g;
    g.T = T; g.H = H; g.W = W;
    g.OH = ceil_div(H, sh_); g.OW = ceil_div(W, sw);
    g.kt = kt; g.kh = kh; g.kw = kw; g.st = st; g.sh = sh_; g.sw = sw; g.pt = pt; g.ph = ph; g.pw = pw;
    const int64_t total = (int64_t)ceil_div(T, st) * g.OH * g.OW * (C / 4);
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HV_ERR_ARG;
    i3d_maxpool_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(x, ldx, y, ldy, g, C / 4, total);
    return hv_check_launch();
}

extern "C" int hv_i3d_head_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* out, int T, int H, int W, int C,
                               float* workspace, int64_t workspace_floats, hipStream_t stream) {
    if (!x || !w || !bias || !out || !workspace) return HV_ERR_ARG;
    if (H != 7 || W != 7 || C != kHeadC || T < 2 || T > HV_I3D_HEAD_MAX_T) return HV_ERR_ARG;
    if (ldx < C || ldx % 4 != 0 || !hv_aligned16(x) || !hv_aligned16(workspace)) return HV_ERR_ARG;
    if (workspace_floats < (int64_t)(T - 1) * kHeadC) return HV_ERR_ARG;
    i3d_head_pool<<<dim3(T - 1), dim3(kThreads), 0, stream>>>(x, ldx, workspace);
    i3d_head_logits<<<dim3((kHeadN + 63) / 64), dim3(64), 0, stream>>>(workspace, w, bias, out, T - 1);
    return hv_check_launch();
}

extern "C" int hv_i3d_preprocess(const void* x, int64_t x_sc, int64_t x_st, int64_t x_sh, int dtype, int T, int H, int W, int RH, int RW,
                                 int rescale, float* y, hipStream_t stream) {
    if (!x || !y || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1)) return HV_ERR_ARG;
    if (T < 1 || T > (1 << 16) || H < 1 || W < 1 || H > (1 << 16) || W > (1 << 16)) return HV_ERR_ARG;
    if (x_sh < W || x_sc < 0 || x_st < 0 || !hv_aligned16(y)) return HV_ERR_ARG;
    // the shorter side goes to 224, the other one keeps the aspect ratio up to the caller's rounding (within one pixel of exact)
    if (RH < 224 || RW < 224 || (RH != 224 && RW != 224) || RH > (1 << 20) || RW > (1 << 20)) return HV_ERR_ARG;
    // a square clip may come with either side at 224: the reference's ceil(H * (224 / H)) is 225 for some H (100, 200, 400, ...)
    if ((H < W && RH != 224) || (W < H && RW != 224)) return HV_ERR_ARG;
    const int64_t total = (int64_t)T * 224 * 224;
    const unsigned blocks = (unsigned)((total + kThreads - 1) / kThreads);
    if (dtype == 0)
        i3d_preprocess_kernel<_Float16><<<dim3(blocks), dim3(kThreads), 0, stream>>>((const _Float16*)x, x_sc, x_st, x_sh, T, H, W, RH, RW, rescale, y);
    else
        i3d_preprocess_kernel<float><<<dim3(blocks), dim3(kThreads), 0, stream>>>((const float*)x, x_sc, x_st, x_sh, T, H, W, RH, RW, rescale, y);
    return hv_check_launch();
}
