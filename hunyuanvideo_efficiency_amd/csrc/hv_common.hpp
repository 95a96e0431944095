// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the HunyuanVideo hot path.
// Wave = 64 lanes everywhere; bf16 values travel as raw 16-bit words and are widened in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define HV_OK 0
#define HV_ERR_ARG (-1)
#define HV_ERR_LAUNCH (-2)

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

typedef uint16_t bf16_t;  // storage type in HBM / LDS

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ float bf2f_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf2f_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }
// round-to-nearest-even f32 -> bf16 (a plain cast lowers to v_cvt_pk_bf16_f32 on gfx950, NaN-safe)
__device__ __forceinline__ bf16_t f2bf(float f) {
    __bf16 h = (__bf16)f;
    return __builtin_bit_cast(bf16_t, h);
}
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}
// round a float to the nearest bf16 value, kept as float (the "bf16-emulated" contract points)
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }

__device__ __forceinline__ void unpack8(const u32x4& w, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf2f_lo(w[i]);
        f[2 * i + 1] = bf2f_hi(w[i]);
    }
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf2(f[2 * i], f[2 * i + 1]);
    return w;
}

// fp16 twins of the bf16 helpers above: raw 16-bit words in memory, fp32 in registers, round to nearest even on the way back
typedef _Float16 h16;
__device__ __forceinline__ float h2f(uint16_t v) { return (float)__builtin_bit_cast(h16, v); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, (h16)f); }
__device__ __forceinline__ float rh(float f) { return (float)(h16)f; }
__device__ __forceinline__ void unpack8h(const u32x4& w, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = h2f((uint16_t)(w[i] & 0xFFFFu));
        f[2 * i + 1] = h2f((uint16_t)(w[i] >> 16));
    }
}
__device__ __forceinline__ u32x4 pack8h(const float (&f)[8]) {
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2h(f[2 * i]) | ((uint32_t)f2h(f[2 * i + 1]) << 16);
    return w;
}

// Butterfly over the 64 lanes of a wave: every lane ends with op folded over all of them, in one fixed order.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
struct WaveAdd {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct WaveMax {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
    __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
};
struct WaveMin {
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
};
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, WaveAdd{}); }   // float, double, uint64
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, WaveMax{}); }   // float, int
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, WaveMin{}); }   // int

__device__ __forceinline__ float gelu_tanh_f(float x) {
    // nn.GELU(approximate="tanh"): 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    float u = k0 * (x + k1 * x * x * x);
    // tanh(u) = 1 - 2/(exp(2u)+1); exp via exp2
    float e = __builtin_amdgcn_exp2f(u * 2.8853900817779268f);  // exp(2u)
    // v_rcp_f32 (1 ulp) instead of an IEEE division (a ~10-instruction expansion per element): the result is rounded to bf16 /
    // fp16 right after, 13+ bits coarser than the reciprocal's error
    float t = 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
    return 0.5f * x * (1.0f + t);
}
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// The 8-bit frame value of the scoring kernels (hv_metrics.hip, hv_lpips.hip), utils/file_utils.py:frames_uint8: x.float();
// (x + 1.0) / 2.0 if rescale; clamp(0, 1); * 255; astype(uint8) - each step rounded to fp32 on its own (the intrinsics keep hipcc
// from contracting the add and a multiply into one FMA).  NaN quantises to 0.
__device__ __forceinline__ uint32_t quantise(float x, int rescale) {
    if (rescale) x = __fmul_rn(__fadd_rn(x, 1.0f), 0.5f);
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    return (uint32_t)(int)__fmul_rn(x, 255.0f);
}

// The fp32-input MFMA block tile of the scoring networks' implicit-GEMM convolutions (hv_lpips.hip, hv_i3d.hip): 128 output rows x 64
// output channels x 32 k per step, four waves of 64 x 32 with two independent 32x32 accumulators each, on v_mfma_f32_32x32x2_f32 (fp32
// in, fp32 accumulate: every output element is one k-ordered fmaf chain, whatever tile it falls in).  LDS tiles are k-major: the 32 lanes
// that share a k read 32 consecutive dwords (conflict-free ds_read_b32); the A rows are 130 dwords long so that a loader's 8 rows x 8
// k-quads of one wave spread over all banks.
namespace f32tile {
constexpr int kThreads = 256;
constexpr int BM = 128, BN = 64, BK = 32;
constexpr int LDA = BM + 2;

// the MFMAs of one staged k-chunk: sA [BK][LDA], sB [BK][BN]; wave tile at rows wm, columns wn
__device__ __forceinline__ void mma_chunk(const float* sA, const float* sB, int wm, int wn, int lr, int lk, f32x16& acc0, f32x16& acc1) {
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks) {
        const int k = ks * 2 + lk;
        const float a0 = sA[k * LDA + wm + lr], a1 = sA[k * LDA + wm + 32 + lr];
        const float b = sB[k * BN + wn + lr];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
    }
}
// C/D map of the 32x32 forms: column = lane & 31, row of register r = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
}  // namespace f32tile

static inline bool hv_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The output-pitch rule of the C ABI (include/hv_kernels.h): rows stored next to each other must not share an address, so a pitch
// below the width written per row is a bad argument once more than one row is written.  A single row has no neighbour and is exempt
// (torch reports arbitrary strides for size-1 dimensions: a [1, N] view may carry stride(0) < N).
static inline bool hv_pitch_ok(int64_t rows, int64_t pitch, int64_t width) { return rows <= 1 || pitch >= width; }
// A block count that dim3 would truncate: grid.x holds at most 2^31 - 1 workgroups.
static inline bool hv_grid_x_ok(int64_t blocks) { return blocks >= 0 && blocks <= 0x7fffffff; }

// Raising a kernel's dynamic-LDS limit is a per-DEVICE attribute: one process may drive several GPUs, so the "already done"
// flag is kept per device ordinal (hipGetDevice is a thread-local read, no driver call).
struct HvPerDeviceOnce { bool done[64] = {}; };
static inline int hv_set_max_lds(HvPerDeviceOnce& once, const void* fn, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return HV_ERR_LAUNCH;
    if (!once.done[dev]) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return HV_ERR_LAUNCH;
        once.done[dev] = true;
    }
    return HV_OK;
}

static inline int hv_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? HV_OK : HV_ERR_LAUNCH;
}

// (lo, hi) fp16 halves of w minus fp32 pivots, widened and subtracted in one v_fma_mix_f32 each (exact for fp16 values and fp16
// pivots; the compiler emits a convert and a subtract): the shifted moments of the GroupNorm statistics at the cost of plain ones
__device__ __forceinline__ f32x2 f16x2_minus(uint32_t w, float plo, float phi) {
    float lo, hi;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(w), "v"(plo));
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(hi) : "v"(w), "v"(phi));
    return f32x2{lo, hi};
}
