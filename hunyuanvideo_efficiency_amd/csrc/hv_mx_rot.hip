// MXFP4 linears, rotated operands (opt-in; include/hv_mx_rot.h holds the contract): the two quantisers of hv_gemm_mx4.hip with a
// block-diagonal Walsh-Hadamard rotation of R = 16 / 64 / 256 consecutive k in front of the quantiser rule.  hv_gemm_mxfp4 consumes
// the result as it is: (A H)(W H)^T = A W^T.
//
// Work split: the unrotated quantisers' - one wave per row, a lane holds the 8 consecutive elements of one 16-byte load, 4 adjacent
// lanes an MX block - so a rotation group is R / 8 = 2, 8 or 32 adjacent lanes, and K % R == 0 gives them the same trips.
//   * stages 0 - 2 pair elements inside the lane: 24 adds / subtracts on its 8 registers.
//   * stage 3 + t pairs lane l with lane l ^ 2^t; the lane with bit t clear needs own + partner, the other one partner - own.  Done
//     literally that is a move, a select or sign flip and an add per element.  Here a lane carries s * y instead of y, s = +-1 its
//     own sign, and every stage is ONE fused multiply-add per element, own + c_t * partner, c_t = +1 in the lower lane and -1 in the
//     upper (constants per lane): the lower lane gets s (y + y'), the upper s (y - y') = -s (y' - y), i.e. its sign flips.  A lane's
//     and its partner's s agree before every stage (they differ in bit t only, and s = (-1)^popcount of the bits below t).  c * p is
//     exact, so the fma rounds once, exactly as the add or subtract would, and rounding is symmetric in sign: bit for bit the
//     contract's values.  The last sign, (-1)^popcount(l & (R / 8 - 1)), rides on the contract's final multiply by 2^-(log2 R / 2).
//   * the partner's value: t = 0, 1 DPP quad_perm, t = 3 DPP row_ror:8, read by the v_fmac_f32 itself - one instruction per element
//     and stage - and t = 2, 4 ds_swizzle in bit mode (xor 4, xor 16; there is no DPP control for either), which goes through the LDS
//     crossbar without touching LDS memory.  No barrier, no __shared__.
// Built without the packed fp32 instructions like hv_gemm_mx4.hip (Makefile): the results are pinned bit for bit.
#include "hv_common.hpp"
#include "hv_ln_row.hpp"
#include "hv_mx4_quant.hpp"
#include "../../include/hv_mx_rot.h"
#include <utility>

namespace {

// One cross-lane stage on a lane's 8 values, f[i] <- f[i] + c * (f[i] of the partner lane).
// DPP form: v_fmac_f32 reads the partner's register through the DPP control.  Written as asm: the compiler keeps a v_mov_b32_dpp in
// front of a v_fmac_f32 it does not fold into.  The 8 instructions touch 8 different registers, and the block opens with the wait states
// a DPP read needs behind a VALU write of its source (2) or of EXEC (5), which the compiler does not count inside asm; a value the
// stage before wrote is 8 instructions old.  Every source lane is in the row and active: bound_ctrl never applies.
#define HV_FMAC_DPP(i, CTRL) "v_fmac_f32_dpp %" #i ", %" #i ", %8 " CTRL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define HV_STAGE_DPP(f, c, CTRL)                                                                                                     \
    asm volatile("s_nop 4\n\t" HV_FMAC_DPP(0, CTRL) HV_FMAC_DPP(1, CTRL) HV_FMAC_DPP(2, CTRL) HV_FMAC_DPP(3, CTRL) HV_FMAC_DPP(4, CTRL)  \
                 HV_FMAC_DPP(5, CTRL) HV_FMAC_DPP(6, CTRL) HV_FMAC_DPP(7, CTRL)                                                     \
                 : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7])                   \
                 : "v"(c))
// ds_swizzle form, bit mode: source lane = ((lane & 0x1F) ^ XOR) inside each half-wave
template <int XOR>
__device__ __forceinline__ void stage_swizzle(float (&f)[8], float c) {
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(f[i]), (XOR << 10) | 0x1F));
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = __builtin_fmaf(p[i], c, f[i]);
}

// The rotation of one group on the R / 8 lanes that hold it.  LOG2R = 4, 6, 8.
template <int LOG2R>
struct Wht {
    static constexpr int NT = LOG2R - 3;      // cross-lane stages
    float c[NT];                              // c[t] = +1 where the lane's bit t is clear, -1 where it is set
    float fin;                                // +-2^-(LOG2R / 2): the orthonormal factor with the lane's accumulated sign

    __device__ __forceinline__ explicit Wht(int lane) {
#pragma unroll
        for (int t = 0; t < NT; ++t) c[t] = __uint_as_float(0x3F800000u | ((uint32_t)(lane >> t) << 31));
        const uint32_t odd = (uint32_t)__builtin_popcount(lane & ((1 << NT) - 1)) & 1u;
        fin = __uint_as_float(((uint32_t)(127 - LOG2R / 2) << 23) | (odd << 31));
    }
    __device__ __forceinline__ void operator()(float (&f)[8]) const {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (!(i & (1 << s))) {
                    const float a = f[i], b = f[i | (1 << s)];
                    f[i] = a + b;
                    f[i | (1 << s)] = a - b;
                }
            }
        }
        static_stages(std::make_integer_sequence<int, NT>{}, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] *= fin;
    }
    template <int... T>
    __device__ __forceinline__ void static_stages(std::integer_sequence<int, T...>, float (&f)[8]) const {
        (stage<T>(f), ...);
    }
    template <int T>
    __device__ __forceinline__ void stage(float (&f)[8]) const {      // partner = lane ^ 2^T
        if constexpr (T == 0) HV_STAGE_DPP(f, c[T], "quad_perm:[1,0,3,2]");
        else if constexpr (T == 1) HV_STAGE_DPP(f, c[T], "quad_perm:[2,3,0,1]");
        else if constexpr (T == 3) HV_STAGE_DPP(f, c[T], "row_ror:8");
        else stage_swizzle<1 << T>(f, c[T]);
    }
};

template <int LOG2R>
__global__ __launch_bounds__(256) void quant_rows_mx4_rot_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ codes,
                                                                  int64_t ldq, uint8_t* __restrict__ scales, int64_t lds, int64_t M,
                                                                  int K) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const Wht<LOG2R> wht(lane);
    const bf16_t* xr = x + row * ldx;
    const int nchunk = K >> 3;              // a multiple of R / 8: the lanes of a group run the same trips
    for (int ch = lane; ch < nchunk; ch += 64) {
        float f[8];
        unpack8(*reinterpret_cast<const u32x4*>(xr + ch * 8), f);
        wht(f);
        uint32_t e;
        const uint32_t w = mx4_quant8(f, e);
        *reinterpret_cast<uint32_t*>(codes + row * ldq + ch * 4) = w;
        if ((lane & 3) == 0) scales[row * lds + (ch >> 2)] = (uint8_t)e;
    }
}

// ln_mod_mx4_kernel (hv_gemm_mx4.hip) operation for operation up to the bf16 rounding, then the rotation of the register-resident
// row in place, slot by slot (the lanes of a group hold it in the same slot c), and the quantiser
template <int MAXC, int LOG2R>
__global__ __launch_bounds__(256) void ln_mod_mx4_rot_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ add,
                                                              const bf16_t* __restrict__ mul, uint8_t* __restrict__ codes, int64_t ldq,
                                                              uint8_t* __restrict__ scales, int64_t lds, int64_t M, int D, int64_t ldx,
                                                              float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const Wht<LOG2R> wht(lane);
    const int nchunk = D >> 3;
    float v[MAXC][8];
    const float mean = wave_sum(ln_load_row<MAXC>(x + row * ldx, lane, nchunk, v)) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = v[c][j] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {                  // nchunk % (R / 8) == 0: taken by whole groups
            float m[8], a[8];
            ln_load_coeffs(mul, add, ch, 0, m, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = rbf((v[c][j] - mean) * rstd * m[j] + a[j]);
            wht(v[c]);
            uint32_t e;
            const uint32_t w = mx4_quant8(v[c], e);
            *reinterpret_cast<uint32_t*>(codes + row * ldq + ch * 4) = w;
            if ((lane & 3) == 0) scales[row * lds + (ch >> 2)] = (uint8_t)e;
        }
    }
}

bool rot_args_ok(const void* x, const void* codes, const void* scales, int64_t M, int K, int64_t ldx, int64_t ldq, int64_t lds, int rot) {
    return mx4_quant_args_ok(x, codes, scales, M, K, ldx, ldq, lds) && (rot == 16 || rot == 64 || rot == 256) && K % rot == 0;
}
// launch(integral_constant<int, log2 rot>)
template <typename Launch>
void rot_dispatch(int rot, Launch launch) {
    if (rot == 16)
        launch(std::integral_constant<int, 4>{});
    else if (rot == 64)
        launch(std::integral_constant<int, 6>{});
    else
        launch(std::integral_constant<int, 8>{});
}

}  // namespace

extern "C" int hv_quant_rows_mxfp4_rot(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, int64_t M, int K,
                                       int rot, hipStream_t stream) {
    if (!rot_args_ok(x, codes, scales, M, K, ldx, ldq, lds, rot)) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    rot_dispatch(rot, [&](auto lg) {
        quant_rows_mx4_rot_kernel<decltype(lg)::value><<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream>>>(
            (const bf16_t*)x, ldx, (uint8_t*)codes, ldq, (uint8_t*)scales, lds, M, K);
    });
    return hv_check_launch();
}

extern "C" int hv_ln_modulate_mxfp4_rot(const void* x, const void* shift, const void* scale, void* codes, int64_t ldq, void* scales,
                                        int64_t lds, int64_t M, int D, int64_t ldx, float eps, int rot, hipStream_t stream) {
    if (!rot_args_ok(x, codes, scales, M, D, ldx, ldq, lds, rot) || D > 4096) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    dim3 grid((unsigned)((M + 3) / 4)), block(256);
    ln_dispatch_maxc(D, [&](auto maxc) {
        rot_dispatch(rot, [&](auto lg) {
            ln_mod_mx4_rot_kernel<decltype(maxc)::value, decltype(lg)::value><<<grid, block, 0, stream>>>(
                (const bf16_t*)x, (const bf16_t*)shift, (const bf16_t*)scale, (uint8_t*)codes, ldq, (uint8_t*)scales, lds, M, D, ldx, eps);
        });
    });
    return hv_check_launch();
}
