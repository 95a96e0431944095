// The MXFP4 quantiser rule of include/hv_gemm_mx4.h as the quantiser kernels share it (hv_gemm_mx4.hip: plain; hv_mx_rot.hip: behind a
// block-Hadamard rotation), and their common argument check.
// Four adjacent lanes hold one block of 32 (8 elements each).  Everything after the block maximum is integer work or an exact fp32
// multiply by a power of two and compares against constants: no rounding happens here that the contract does not name.
#pragma once
#include "hv_common.hpp"
#include "../../include/hv_gemm_mx4.h"

__device__ __forceinline__ uint32_t e2m1_code(float x, float mul) {
    const float v = fabsf(x) * mul;
    const uint32_t c = (uint32_t)(v > 0.25f) + (uint32_t)(v >= 0.75f) + (uint32_t)(v > 1.25f) + (uint32_t)(v >= 1.75f) +
                       (uint32_t)(v > 2.5f) + (uint32_t)(v >= 3.5f) + (uint32_t)(v > 5.0f);
    return c ? c | ((__float_as_uint(x) >> 28) & 8u) : 0u;
}
// the largest magnitude of a lane's 8 values, as fp32 bits (non-negative floats order as integers)
__device__ __forceinline__ uint32_t mx4_amax8(const float (&f)[8]) {
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, __float_as_uint(f[j]) & 0x7FFFFFFFu);
    return amax;
}
// 8 values of a lane + the block's largest magnitude -> its 4 code bytes; e = the block's E8M0 byte
__device__ __forceinline__ uint32_t mx4_codes8(const float (&f)[8], uint32_t amax, uint32_t& e) {
    const uint32_t E = amax >> 23;
    e = E > 2 ? E - 2 : 0;
    const float mul = __uint_as_float((254u - e) << 23);         // 2^(127 - e): e <= 253, a normal number
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= e2m1_code(f[j], mul) << (4 * j);
    return w;
}
// the same where four ADJACENT lanes hold the block (the row quantisers: one wave per row, a lane = one 16-byte load)
__device__ __forceinline__ uint32_t mx4_quant8(const float (&f)[8], uint32_t& e) {
    uint32_t amax = mx4_amax8(f);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
    return mx4_codes8(f, amax, e);
}

static inline bool mx4_quant_args_ok(const void* x, const void* codes, const void* scales, int64_t M, int K, int64_t ldx, int64_t ldq,
                                     int64_t lds) {
    if (!x || !codes || !scales || M < 0 || K <= 0 || (K % HV_MX4_BLOCK) || (ldx & 7) || (ldq & 15) || !hv_aligned16(codes)) return false;
    return hv_pitch_ok(M, ldq, K / 2) && hv_pitch_ok(M, lds, K / HV_MX4_BLOCK) && hv_grid_x_ok((M + 3) / 4);
}
