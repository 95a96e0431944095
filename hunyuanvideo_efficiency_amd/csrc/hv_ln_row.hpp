// The row-in-registers pieces of the LayerNorm kernels (hv_rowwise.hip: bf16 and e4m3 outputs; hv_gemm_mx4.hip: MXFP4 output).
// One wave per row, D <= 4096, D % 8 == 0.  A lane owns the 8-element chunks lane, lane + 64, ... of its row: chunk slot c of a lane
// is chunk lane + 64 c.
#pragma once
#include "hv_common.hpp"
#include <type_traits>

// row -> v (the slots behind the row's end stay unwritten); returns the lane's sum of its elements
template <int MAXC>
__device__ __forceinline__ float ln_load_row(const bf16_t* xr, int lane, int nchunk, float (&v)[MAXC][8]) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
            unpack8(*reinterpret_cast<const u32x4*>(xr + ch * 8), v[c]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[c][j];
        }
    }
    return s;
}
// the coefficients of chunk ch: m = bf16(1 + mul) (mode 0) or mul (mode 1), 1 without mul; a = add, 0 without add
__device__ __forceinline__ void ln_load_coeffs(const bf16_t* mul, const bf16_t* add, int ch, int mode,
                                               float (&m)[8], float (&a)[8]) {
    if (mul) {
        unpack8(*reinterpret_cast<const u32x4*>(mul + ch * 8), m);
        if (mode == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = rbf(1.0f + m[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = 1.0f;
    }
    if (add) {
        unpack8(*reinterpret_cast<const u32x4*>(add + ch * 8), a);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = 0.0f;
    }
}

// The row-length ladder of the LN kernels: launch(integral_constant<int, MAXC>) with the smallest MAXC whose 512 * MAXC
// elements hold a row of D.
template <typename Launch>
static inline void ln_dispatch_maxc(int D, Launch launch) {
    if (D <= 512)
        launch(std::integral_constant<int, 1>{});
    else if (D <= 2048)
        launch(std::integral_constant<int, 4>{});
    else if (D <= 3072)
        launch(std::integral_constant<int, 6>{});
    else
        launch(std::integral_constant<int, 8>{});
}
