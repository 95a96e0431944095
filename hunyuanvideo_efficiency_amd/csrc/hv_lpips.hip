// LPIPS (AlexNet trunk, version 0.1, linear layers, spatial average) on the device: the reference's lpips.LPIPS(net="alex") as its
// evaluation/compute_metrics.py:43-62 calls it (rebuttal/common_metrics_on_video_quality/lpips/lpips.py:112-144,147-167,
// lpips/__init__.py:13-15, lpips/pretrained_networks.py:56-94), in fp32 like the reference.
//
//   lpips_conv_kernel<Video<T>>   conv 3->64 k11 s4 p2 + bias + ReLU straight from the two [C,T,H,W] videos: the loader quantises each
//                                 value to its 8-bit frame value (frames_uint8, as hv_metrics.hip) and looks it up in the host's
//                                 lut[3][256] (the fp32 input scaling of the reference, bit for bit); no scaled copy reaches HBM
//   lpips_conv_kernel<Feature>    conv k x k stride 1 + bias + ReLU on channels-last fp32 features [image][h][w][C]
//   lpips_maxpool_kernel          3x3 stride 2 (floor) on channels-last fp32
//   lpips_distance_kernel / fold  per pixel: both channel norms, sum_c lin[c] (f0/(|f0|+1e-10) - f1/(|f1|+1e-10))^2; fp64 workgroup
//                                 partials to a workspace, one wave per frame folds them in a fixed order (no atomics)
//
// The convolutions are implicit GEMMs on the fp32-input MFMA block tile of hv_common.hpp (f32tile: 128 output pixels, across image
// boundaries, x 64 output channels x 32 k; every output element is one k-ordered fmaf chain, whatever tile it falls in).  The loader's
// 8 rows x 8 k-quads of one wave spread over all LDS banks (2-way at most, free for ds_write_b32).  The next k-chunk is fetched into
// registers while the MFMAs of this one run.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"

namespace {

using namespace f32tile;
constexpr int kK1 = 3 * 11 * 11;             // 363: k = (c * 11 + ky) * 11 + kx of the first layer, zero-padded to 384
constexpr int kMaxC = 384;                   // widest tap
constexpr int kDistMaxWg = 256;              // distance workgroups per frame

struct Strides {
    int64_t sc, st, sh;
};

// what a thread keeps of "its" output pixels across the k loop
struct Row {
    int img, iy0, ix0;                       // image, top-left input coordinate of the window (iy0 very negative: row beyond M)
};
__device__ __forceinline__ Row decode_row(int64_t m, int64_t M, int OH, int OW, int stride, int pad) {
    Row r;
    if (m >= M) {
        r.img = 0; r.iy0 = -(1 << 28); r.ix0 = 0;
        return r;
    }
    const int pix = OH * OW;
    r.img = (int)(m / pix);
    const int p = (int)(m - (int64_t)r.img * pix);
    const int oy = p / OW;
    r.iy0 = oy * stride - pad;
    r.ix0 = (p - oy * OW) * stride - pad;
    return r;
}

// ---- A-tile loaders ---------------------------------------------------------------------------------------------------------------
// channels-last fp32 features; k = (ky * KS + kx) * Cin + ci, Cin % 32 == 0: one k-chunk is 32 consecutive channels of one tap.
// Thread (row = tid >> 3 (+32, +64, +96), quad = tid & 7) moves one float4: 8 lanes read the 128 contiguous bytes of a pixel.
struct Feature {
    const float* x;
    int H, W, Cin, KS;
    struct State {                           // per thread, across the k loop (the loader itself is the kernel argument)
        Row rows[4];
        f32x4 v[4];
    };

    __device__ __forceinline__ void init(State& st, int64_t m0, int64_t M, int OH, int OW, int pad, int tid, const float*) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) st.rows[i] = decode_row(m0 + (tid >> 3) + 32 * i, M, OH, OW, 1, pad);
    }
    __device__ __forceinline__ void fetch(State& st, int kc, int tid) const {
        Row (&rows)[4] = st.rows;
        f32x4 (&v)[4] = st.v;
        const int k0 = kc * BK;
        const int tap = k0 / Cin, ci = k0 - tap * Cin + (tid & 7) * 4;
        const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int iy = rows[i].iy0 + ky, ix = rows[i].ix0 + kx;
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (iy >= 0 && iy < H && ix >= 0 && ix < W)
                v[i] = *(const f32x4*)(x + (((int64_t)rows[i].img * H + iy) * W + ix) * Cin + ci);
        }
    }
    __device__ __forceinline__ void store(const State& st, float* sA, int tid) const {
        const f32x4 (&v)[4] = st.v;
        const int q = (tid & 7) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sA[(q + j) * LDA + (tid >> 3) + 32 * i] = v[i][j];
    }
};

// the two videos, [C,T,H,W] fp16 or fp32 with element strides; image i < T is frame i of `a`, image T + i frame i of `b`.
// Thread (row = tid & 127, half = tid >> 7) gathers 16 consecutive k of its row; k is uniform over a wave.
template <typename T>
struct Video {
    const T *a, *b;
    Strides sa, sb;
    int Tn, H, W, rescale;
    struct State {
        const T* base;                       // this thread's frame
        int64_t sc, sh;
        Row row;
        const float* lut;                    // LDS copy of lut[3][256]
        float v[16];
    };

    __device__ __forceinline__ void init(State& st, int64_t m0, int64_t M, int OH, int OW, int pad, int tid, const float* s_lut) const {
        st.row = decode_row(m0 + (tid & 127), M, OH, OW, 4, pad);
        const bool second = st.row.img >= Tn;
        const Strides s = second ? sb : sa;
        st.sc = s.sc; st.sh = s.sh;
        st.base = (second ? b : a) + (int64_t)(second ? st.row.img - Tn : st.row.img) * s.st;
        st.lut = s_lut;
    }
    __device__ __forceinline__ void fetch(State& st, int kc, int tid) const {
        const Row row = st.row;
        float (&v)[16] = st.v;
        const int k0 = kc * BK + (tid >> 7) * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int k = k0 + j;
            const int c = k / 121, r = k - c * 121;
            const int ky = r / 11, kx = r - ky * 11;
            const int iy = row.iy0 + ky, ix = row.ix0 + kx;
            v[j] = 0.f;
            if (k < kK1 && iy >= 0 && iy < H && ix >= 0 && ix < W)
                v[j] = st.lut[c * 256 + quantise((float)st.base[c * st.sc + iy * st.sh + ix], rescale)];
        }
    }
    __device__ __forceinline__ void store(const State& st, float* sA, int tid) const {
#pragma unroll
        for (int j = 0; j < 16; ++j) sA[((tid >> 7) * 16 + j) * LDA + (tid & 127)] = st.v[j];
    }
};

// y[m][n] = relu(bias[n] + sum_k A[m][k] w[k][n]); w is [nk * 32][Cout] (k-major, zero rows behind K), y channels-last [M][Cout]
template <typename Loader>
__global__ __launch_bounds__(kThreads) void lpips_conv_kernel(const Loader ld, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y, const float* __restrict__ lut, int64_t M, int OH,
                                                             int OW, int pad, int Cout, int nk) {
    __shared__ float sA[BK * LDA];
    __shared__ __attribute__((aligned(16))) float sB[BK * BN];
    __shared__ float s_lut[3 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntn = Cout / BN;
    const int64_t m0 = (int64_t)(blockIdx.x / ntn) * BM;          // the column tiles of one row tile are neighbours in the grid
    const int n0 = (int)(blockIdx.x % ntn) * BN;
    if (lut != nullptr) {
        for (int i = tid; i < 3 * 256; i += kThreads) s_lut[i] = lut[i];
        __syncthreads();
    }
    typename Loader::State st;
    ld.init(st, m0, M, OH, OW, pad, tid, s_lut);

    const int bk = tid >> 4, bn = (tid & 15) * 4;                 // B: rows bk and bk + 16 of the chunk, 4 columns
    const float* wp = w + (int64_t)bk * Cout + n0 + bn;
    f32x4 vb0, vb1;
    auto fetch_b = [&](int kc) {
        const float* p = wp + (int64_t)kc * BK * Cout;
        vb0 = *(const f32x4*)p;
        vb1 = *(const f32x4*)(p + (int64_t)16 * Cout);
    };

    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 32;
    const int lr = lane & 31, lk = lane >> 5;
    f32x16 acc0 = {}, acc1 = {};
    ld.fetch(st, 0, tid);
    fetch_b(0);
    for (int kc = 0; kc < nk; ++kc) {
        ld.store(st, sA, tid);
        *(f32x4*)(sB + bk * BN + bn) = vb0;
        *(f32x4*)(sB + (bk + 16) * BN + bn) = vb1;
        __syncthreads();
        if (kc + 1 < nk) {
            ld.fetch(st, kc + 1, tid);
            fetch_b(kc + 1);
        }
        mma_chunk(sA, sB, wm, wn, lr, lk, acc0, acc1);
        __syncthreads();
    }

    const int n = n0 + wn + lr;
    const float bv = bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = acc_row(r, lk);
        const int64_t ma = m0 + wm + row, mb = ma + 32;
        if (ma < M) y[ma * Cout + n] = fmaxf(acc0[r] + bv, 0.f);
        if (mb < M) y[mb * Cout + n] = fmaxf(acc1[r] + bv, 0.f);
    }
}

// ---- maxpool 3x3 stride 2 ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lpips_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C4,
                                                                int OH, int OW, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    int64_t p = i / C4;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const int64_t img = p / OH;
    const f32x4* src = (const f32x4*)x + ((img * H + oy * 2) * W + ox * 2) * C4 + c;
    f32x4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const f32x4 v = src[((int64_t)dy * W + dx) * C4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
        }
    ((f32x4*)y)[i] = m;
}

// ---- layer distance ---------------------------------------------------------------------------------------------------------------
// f: [2T][P][C]; frame t compares image t with image T + t.  One wave per pixel (lanes along C, <= 6 channels each); workgroup g of
// a frame takes pixels g * 4 + wave, + 4 * nwg, ...: the partition depends on P alone, so a frame's bits do not depend on T.
__global__ __launch_bounds__(kThreads) void lpips_distance_kernel(const float* __restrict__ f, const float* __restrict__ lin, int T, int64_t P,
                                                                 int C, double* __restrict__ part) {
    __shared__ double s_red[kThreads / 64];
    const int t = blockIdx.y, nwg = gridDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* f0 = f + (int64_t)t * P * C;
    const float* f1 = f + (int64_t)(T + t) * P * C;
    constexpr int R = kMaxC / 64;
    float lw[R];
#pragma unroll
    for (int j = 0; j < R; ++j) lw[j] = lane + 64 * j < C ? lin[lane + 64 * j] : 0.f;
    double sum = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * 4 + wave; p < P; p += (int64_t)nwg * 4) {
        float a[R], b[R];
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int c = lane + 64 * j;
            a[j] = c < C ? f0[p * C + c] : 0.f;
            b[j] = c < C ? f1[p * C + c] : 0.f;
            sa += (double)a[j] * (double)a[j];
            sb += (double)b[j] * (double)b[j];
        }
        sa = wave_sum(sa);
        sb = wave_sum(sb);
        const float da = (float)sqrt(sa) + 1e-10f, db = (float)sqrt(sb) + 1e-10f;   // all-zero pixel: 0 / 1e-10 = 0
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const float d = a[j] / da - b[j] / db;
            sum += (double)(lw[j] * (d * d));
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) s_red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double s = s_red[0];
        for (int wv = 1; wv < kThreads / 64; ++wv) s += s_red[wv];
        part[(int64_t)t * nwg + blockIdx.x] = s;
    }
}

// one wave per frame: lane l adds partials l, l + 64, ... in order, then the butterfly
__global__ __launch_bounds__(64) void lpips_distance_fold(const double* __restrict__ part, int nwg, int layer, double* __restrict__ out) {
    const int t = blockIdx.x, l = threadIdx.x;
    double s = 0.0;
    for (int k = l; k < nwg; k += 64) s += part[(int64_t)t * nwg + k];
    s = wave_sum(s);
    if (l == 0) out[t * 5 + layer] = s;
}

inline int dist_wgs(int64_t P) {
    const int64_t n = (P + 63) / 64;
    return (int)(n < 1 ? 1 : n > kDistMaxWg ? kDistMaxWg : n);
}

template <typename Loader>
int launch_conv(const Loader& ld, const float* w, const float* bias, float* y, const float* lut, int64_t M, int OH, int OW, int pad, int Cout,
                int nk, hipStream_t stream) {
    const int64_t blocks = (M + BM - 1) / BM * (Cout / BN);
    if (blocks > 0x7fffffff) return HV_ERR_ARG;
    lpips_conv_kernel<Loader><<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(ld, w, bias, y, lut, M, OH, OW, pad, Cout, nk);
    return hv_check_launch();
}

template <typename T>
int launch_conv1(const void* a, Strides sa, const void* b, Strides sb, int Tn, int H, int W, int rescale, const float* lut, const float* w,
                 const float* bias, float* y, hipStream_t stream) {
    Video<T> ld;
    ld.a = (const T*)a; ld.b = (const T*)b; ld.sa = sa; ld.sb = sb;
    ld.Tn = Tn; ld.H = H; ld.W = W; ld.rescale = rescale;
    const int OH = (H + 4 - 11) / 4 + 1, OW = (W + 4 - 11) / 4 + 1;
    return launch_conv(ld, w, bias, y, lut, (int64_t)2 * Tn * OH * OW, OH, OW, 2, 64, (kK1 + BK - 1) / BK, stream);
}

}  // namespace

extern "C" int hv_lpips_conv1_f32(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st,
                                  int64_t b_sh, int dtype, int T, int H, int W, int rescale, const float* lut, const float* w,
                                  const float* bias, float* y, hipStream_t stream) {
    if (!a || !b || !lut || !w || !bias || !y || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1)) return HV_ERR_ARG;
    if (T < 1 || T > 32767 || H < 31 || W < 31 || H > (1 << 16) || W > (1 << 16)) return HV_ERR_ARG;
    if (a_sh < W || b_sh < W || a_sc < 0 || a_st < 0 || b_sc < 0 || b_st < 0) return HV_ERR_ARG;
    if (!hv_aligned16(w)) return HV_ERR_ARG;
    const Strides sa{a_sc, a_st, a_sh}, sb{b_sc, b_st, b_sh};
    if (dtype == 0) return launch_conv1<_Float16>(a, sa, b, sb, T, H, W, rescale, lut, w, bias, y, stream);
    return launch_conv1<float>(a, sa, b, sb, T, H, W, rescale, lut, w, bias, y, stream);
}

extern "C" int hv_lpips_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                                   int ksize, int pad, hipStream_t stream) {
    if (!x || !w || !bias || !y || N < 1 || H < 1 || W < 1 || H > (1 << 16) || W > (1 << 16)) return HV_ERR_ARG;
    if (Cin < BK || Cin % BK != 0 || Cin > 4096 || Cout < BN || Cout % BN != 0 || Cout > 4096) return HV_ERR_ARG;
    if (ksize < 1 || ksize > 11 || pad < 0 || pad >= ksize) return HV_ERR_ARG;
    const int OH = H + 2 * pad - ksize + 1, OW = W + 2 * pad - ksize + 1;
    if (OH < 1 || OW < 1 || (int64_t)N * H * W > 0x7fffffff || (int64_t)N * OH * OW > 0x7fffffff) return HV_ERR_ARG;
    if (!hv_aligned16(x) || !hv_aligned16(w)) return HV_ERR_ARG;
    Feature ld;
    ld.x = x; ld.H = H; ld.W = W; ld.Cin = Cin; ld.KS = ksize;
    return launch_conv(ld, w, bias, y, nullptr, (int64_t)N * OH * OW, OH, OW, pad, Cout, ksize * ksize * Cin / BK, stream);
}

extern "C" int hv_lpips_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream) {
    if (!x || !y || N < 1 || H < 3 || W < 3 || H > (1 << 16) || W > (1 << 16) || C < 4 || C % 4 != 0 || C > 4096) return HV_ERR_ARG;
    if (!hv_aligned16(x) || !hv_aligned16(y)) return HV_ERR_ARG;
    const int OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    const int64_t total = (int64_t)N * OH * OW * (C / 4);
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffff) return HV_ERR_ARG;
    lpips_maxpool_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, stream>>>(x, y, H, W, C / 4, OH, OW, total);
    return hv_check_launch();
}

extern "C" int64_t hv_lpips_distance_workspace_bytes(int T, int64_t P) {
    if (T < 1 || T > 65535 || P < 1) return 0;
    return (int64_t)T * dist_wgs(P) * 8;
}

extern "C" int hv_lpips_distance_f32(const float* f, const float* lin, int T, int64_t P, int C, int layer, double* out, void* workspace,
                                     int64_t workspace_bytes, hipStream_t stream) {
    if (!f || !lin || !out || !workspace || T < 1 || T > 65535 || P < 1 || C < 1 || C > kMaxC || layer < 0 || layer > 4) return HV_ERR_ARG;
    if (((uintptr_t)workspace & 7) != 0 || workspace_bytes < hv_lpips_distance_workspace_bytes(T, P)) return HV_ERR_ARG;
    const int nwg = dist_wgs(P);
    lpips_distance_kernel<<<dim3(nwg, T), dim3(kThreads), 0, stream>>>(f, lin, T, P, C, (double*)workspace);
    lpips_distance_fold<<<dim3(T), dim3(64), 0, stream>>>((const double*)workspace, nwg, layer, out);
    return hv_check_launch();
}
