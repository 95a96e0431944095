// The output-tile order of the GEMM main loops (hv_gemm.hip, hv_gemm_mx4.hip) and the pointer types of the LDS-DMA builtin.
#pragma once
#include "hv_common.hpp"

constexpr int GROUP_M = 4;                       // M tiles per band of the tile order (2 ~ 4 > 8 > 16: DESIGN.md section 7)

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// XCD-aware tile mapping (bijective for any grid size): workgroup -> linear tile index, so that each XCD (workgroup id mod 8) gets a
// contiguous chunk of tiles
__device__ __forceinline__ int xcd_linear_tile() {
    const int nwg = gridDim.x;
    const int bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// banded tile order: linear index -> (tm, tn), M fastest inside a band of GROUP_M M-tiles (the last band may be shorter)
struct TileMN { int tm, tn; };
__device__ __forceinline__ TileMN tile_of(int lin, int tiles_m, int tiles_n) {
    const int band = lin / (GROUP_M * tiles_n), rem = lin % (GROUP_M * tiles_n);
    const int band_m0 = band * GROUP_M;
    const int gm = min(GROUP_M, tiles_m - band_m0);
    return TileMN{band_m0 + rem % gm, rem / gm};
}
