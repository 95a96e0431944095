// What the block-scaled GEMM main loops (hv_gemm_mx4.hip, hv_gemm_mx6.hip) share: the argument block, the deal of W rows to LDS rows
// that makes a lane own 8 consecutive n, the bf16 epilogue over the 8 x 4 accumulators of a 128 x 64 wave tile, and the host-side
// checks of everything that does not depend on the element format.
#pragma once
#include "hv_common.hpp"
#include <type_traits>
#include <utility>

struct MxGemmArgs {
    const uint8_t *A, *As, *W, *Ws;
    int64_t lda, ldas, ldw, ldws;
    const uint16_t* bias;
    int M, N, K;
    uint16_t* out0; int64_t ld0; int act0;
    int n_split;
    uint16_t* out1; int64_t ld1; int act1;
    const uint16_t* gate;
    const uint16_t* res; int64_t ld_res;
    int tiles_m, tiles_n;
};

template <int... I, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }

// W row (inside the 256-row tile) held by LDS row lr = wn * 64 + ni * 16 + i
__device__ __forceinline__ int w_tile_row(int lr) {
    const int wn = lr >> 6, ni = (lr >> 4) & 3, i = lr & 15;
    return wn * 64 + (ni >> 1) * 32 + (i >> 2) * 8 + (ni & 1) * 4 + (i & 3);
}

// bf16 epilogue of hv_gemm.hip (bias, activation on the rounded value, gated residual, column split), 8 consecutive n per lane
__device__ __forceinline__ void mx_epilogue(const MxGemmArgs& g, f32x4 (&acc)[8][4], int mrow0, int ncol0, int fq) {
    int64_t orow[8];                        // clamped rows are loaded, never stored
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) orow[mi] = min(mrow0 + mi * 16, g.M - 1);
#pragma unroll
    for (int np = 0; np < 2; ++np) {
        const int n = ncol0 + np * 32 + fq * 8;
        if (n >= g.N) continue;
        float b[8], gt[8];
        u32x4 rraw[8];
        if (g.res) {
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) rraw[mi] = *reinterpret_cast<const u32x4*>(g.res + orow[mi] * g.ld_res + n);
        }
        if (g.bias) unpack8(*reinterpret_cast<const u32x4*>(g.bias + n), b);
        else {
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = 0.f;
        }
        if (g.gate) unpack8(*reinterpret_cast<const u32x4*>(g.gate + n), gt);
        const bool second = n >= g.n_split;
        uint16_t* obase = second ? g.out1 + (n - g.n_split) : g.out0 + n;
        const int64_t ldo = second ? g.ld1 : g.ld0;
        const int act = second ? g.act1 : g.act0;
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[mi][2 * np][r] + b[r];
                v[4 + r] = acc[mi][2 * np + 1][r] + b[4 + r];
            }
            if (act == 1) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = gelu_tanh_f(rbf(v[j]));
            } else if (act == 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = silu_f(rbf(v[j]));
            }
            if (g.res) {
                float rs[8];
                unpack8(rraw[mi], rs);
                if (g.gate) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = rs[j] + rbf(rbf(v[j]) * gt[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = rs[j] + rbf(v[j]);
                }
            }
            if (mrow0 + mi * 16 < g.M) *reinterpret_cast<u32x4*>(obase + orow[mi] * ldo) = pack8(v);
        }
    }
}

// Host side: the refusals both GEMMs share (everything but the reduction length), then the argument block for 256 x 256 tiles.
// Code rows are DMA sources of 16-byte chunks and tile offsets are 32-bit; a stage reads a row's four scale bytes as one dword.
static inline bool mx_gemm_args(MxGemmArgs& g, const void* A_codes, int64_t lda, const void* A_scales, int64_t ldas, const void* W_codes,
                                int64_t ldw, const void* W_scales, int64_t ldws, const void* bias, int M, int N, int K, void* out0,
                                int64_t ld0, int act0, int n_split, void* out1, int64_t ld1, int act1, const void* gate, const void* res,
                                int64_t ld_res) {
    if (!A_codes || !A_scales || !W_codes || !W_scales || !out0 || M < 0 || N <= 0 || (N & 7)) return false;
    if (!hv_aligned16(A_codes) || !hv_aligned16(W_codes) || (lda & 15) || (ldw & 15) || lda < 0 || ldw < 0 || lda > (1 << 23) ||
        ldw > (1 << 23))
        return false;
    if (((uintptr_t)A_scales & 3) || ((uintptr_t)W_scales & 3) || (ldas & 3) || (ldws & 3) || (ld0 & 7)) return false;
    if (n_split <= 0 || n_split > N) n_split = N;
    if (n_split < N && (!out1 || (n_split & 7) || (ld1 & 7))) return false;
    if ((gate && !res) || (res && (ld_res & 7))) return false;
    if (act0 < 0 || act0 > 2 || act1 < 0 || act1 > 2) return false;
    if (!hv_pitch_ok(M, ld0, n_split) || (n_split < N && !hv_pitch_ok(M, ld1, N - n_split))) return false;
    g.A = (const uint8_t*)A_codes; g.As = (const uint8_t*)A_scales; g.W = (const uint8_t*)W_codes; g.Ws = (const uint8_t*)W_scales;
    g.lda = lda; g.ldas = ldas; g.ldw = ldw; g.ldws = ldws;
    g.bias = (const uint16_t*)bias; g.M = M; g.N = N; g.K = K;
    g.out0 = (uint16_t*)out0; g.ld0 = ld0; g.act0 = act0; g.n_split = n_split;
    g.out1 = (uint16_t*)out1; g.ld1 = ld1; g.act1 = act1;
    g.gate = (const uint16_t*)gate; g.res = (const uint16_t*)res; g.ld_res = ld_res;
    g.tiles_m = (int)(((int64_t)M + 255) / 256);
    g.tiles_n = (N + 255) / 256;
    return hv_grid_x_ok((int64_t)g.tiles_m * g.tiles_n);
}
