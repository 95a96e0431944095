// Linear temporal interpolation of a channels-last activation [T, HW, C]: the fork's t_ops interpolation with interp_mode "trilinear"
// (unet_causal_3d_blocks.py:853-911: F.interpolate(scale_factor=(s,1,1), mode="trilinear", align_corners=False); H and W have scale 1,
// so only T is interpolated).  The nearest mode is hv_temporal_resample_f16 (hv_vae.hip), which stays as it is.
//
//   temporal_interp_kernel   a lane owns 8 channels (one 16-byte vector) of one pixel and walks `walk` consecutive source intervals
//                            [k, k + 1] of it.  Interval k feeds the output frames t with t0 == k: lo(k) <= t < hi(k),
//                            lo(0) = 0, lo(k) = s k + s / 2, hi(k) = lo(k + 1), hi(T_in - 1) = T_in s (s frames each, but for the
//                            clamped ends).  The lane loads x[k + 1] once, writes every frame of the interval from the two
//                            vectors it holds and keeps x[k + 1] as the next interval's x[k]: a source vector is read 1 + 1 / walk times, not twice per
//                            output.  The host picks walk = 8 once the launch stays deep enough to fill the machine, less for small
//                            planes.  The arithmetic of an output depends on (t, s) only, so the bits do not depend on `walk`.
//                            Frames with lambda == 0 (and all of the last interval, where t1 == t0) are vector copies.
#include "hv_common.hpp"
#include "../../include/hv_temporal.h"

namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(8))) float f32x8;

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 8192;                 // the grid cap of the streaming kernels (hv_vae.hip grid_for); the loop strides past it
constexpr int kMaxWalk = 8;                      // source intervals a lane walks at most
constexpr int64_t kDeep = (int64_t)kMaxBlocks * kThreads;      // lanes of a full grid: a longer walk must leave at least this many

__global__ __launch_bounds__(kThreads) void temporal_interp_kernel(const uint16_t* __restrict__ x, int64_t ldx, uint16_t* __restrict__ out,
                                                                   int64_t ldo, int t_in, int64_t hw, int c8, int s, int walk,
                                                                   int64_t total) {
    const int64_t fs = hw * ldx;                 // elements between two source frames
    const float den = (float)(2 * (int64_t)s);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % c8);
        const int64_t row = idx / c8, p = row % hw;
        const int k0 = (int)(row / hw) * walk, k1 = k0 + min(walk, t_in - k0);
        const uint16_t* src = x + p * ldx + c * 8;
        uint16_t* dst = out + p * ldo + c * 8;
        uint4 a = *reinterpret_cast<const uint4*>(src + (int64_t)k0 * fs);
        for (int k = k0; k < k1; ++k) {
            const bool last = k == t_in - 1;
            const uint4 b = last ? a : *reinterpret_cast<const uint4*>(src + (int64_t)(k + 1) * fs);
            const int64_t lo = k == 0 ? 0 : (int64_t)s * k + s / 2;
            const int64_t hi = last ? (int64_t)s * t_in : (int64_t)s * (k + 1) + s / 2;
            const f32x8 af = __builtin_convertvector(__builtin_bit_cast(f16x8, a), f32x8);      // in registers: no addressable copy
            const f32x8 bf = __builtin_convertvector(__builtin_bit_cast(f16x8, b), f32x8);
            for (int64_t t = lo; t < hi; ++t) {
                const int64_t num = max(2 * t + 1 - s, (int64_t)0);
                const int r = (int)(num - 2 * (int64_t)s * k);          // num mod 2s: t0 == k inside this interval
                uint4 o = a;
                if (r != 0 && !last) {
                    const float lam = __fdiv_rn((float)r, den), w0 = 1.0f - lam;
                    f32x8 y;
#pragma unroll
                    for (int j = 0; j < 8; ++j) y[j] = fmaf(lam, bf[j], w0 * af[j]);
                    o = __builtin_bit_cast(uint4, __builtin_convertvector(y, f16x8));
                }
                *reinterpret_cast<uint4*>(dst + t * hw * ldo) = o;
            }
            a = b;
        }
    }
}

}  // namespace

extern "C" int hv_temporal_interp_f16(const void* x, int64_t ldx, void* out, int64_t ldo, int T_in, int64_t HW, int C, int s,
                                      hipStream_t stream) {
    if (!x || !out || T_in <= 0 || HW <= 0 || C <= 0 || (C & 7) || (ldx & 7) || (ldo & 7) || s < 1 ||
        (((uintptr_t)x | (uintptr_t)out) & 15))
        return HV_ERR_ARG;
    if ((int64_t)T_in * s > 0x7fffffff) return HV_ERR_ARG;
    const int t_out = T_in * s, c8 = C / 8;
    if (HW > INT64_MAX / ((int64_t)t_out * c8) || !hv_pitch_ok((int64_t)t_out * HW, ldo, C)) return HV_ERR_ARG;
    const int64_t plane = HW * c8;               // lanes per walked chunk of intervals (<= t_out * HW * c8: fits)
    int walk = 1;
    while (walk < kMaxWalk && ((int64_t)T_in + 2 * walk - 1) / (2 * walk) >= kDeep / plane + (kDeep % plane != 0)) walk *= 2;
    const int64_t total = (((int64_t)T_in + walk - 1) / walk) * plane;
    const int64_t blocks = (total + kThreads - 1) / kThreads;
    temporal_interp_kernel<<<dim3((unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks)), dim3(kThreads), 0, stream>>>(
        (const uint16_t*)x, ldx, (uint16_t*)out, ldo, T_in, HW, c8, s, walk, total);
    return hv_check_launch();
}
