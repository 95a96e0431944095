// Video tensor [C,T,H,W] (fp16 / fp32) -> raw YUV 4:2:0 frames, the mirror image of hv_yuv.hip, in one pass: the 8-bit RGB frame never
// reaches memory.  The rule is stated in include/hv_yuv_write.h: the quantiser of the scoring kernels (hv_common.hpp: quantise), BT.601
// limited range in 20 fractional bits (int32, no clamp needed), chroma of a 2 x 2 block from its top-left pixel or from the four
// pixels' sums, the layouts I420 / YV12 / NV12 of hv_kernels.h.
//
//   yuv_write_kernel<E, VEC>   a thread owns 8 pixels of two adjacent rows, which share their four chroma samples (the unit of
//                              yuv_copy_kernel).  VEC loads 16 bytes per channel row (fp32: two of them) and stores 2 x 8 bytes of Y
//                              and 2 x 4 bytes (NV12: 8 bytes interleaved) of chroma; without VEC (W % 8 != 0: rows then start at odd
//                              8-byte phases; or an unaligned input, stride or destination) the same run is read element by element and
//                              written byte by byte.
//
// A streaming kernel: grid.x strides over the units of a frame (at most 2048 workgroups over the whole grid), grid.y over the frames.
// Input offsets and frame offsets of the output are 64-bit (a 1080p file passes 2^31 bytes at frame 691); offsets inside one output
// frame fit 32 bits (W, H <= HV_YUV_MAX_SIDE).  No atomics; every output byte is written once.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"
#include "../../include/hv_yuv_write.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWgs = 2048;
constexpr int kRun = 8;                      // pixels of one row a thread owns

struct In {
    const void* x;
    int64_t sc, st, sh;
    int C, rescale;
};

struct Out {
    uint8_t* raw;
    int64_t pitch;                           // bytes of one frame: W * H * 3 / 2
    int W, H, nv12, chroma;
    uint32_t u_off, v_off;                   // first byte of U and V inside a frame (NV12: of the pair and of its second byte)
    int c_ld, c_step;                        // bytes between chroma rows, between chroma samples of one plane
};

__host__ Out make_out(void* raw, int layout, int chroma, int W, int H) {
    Out o;
    o.raw = (uint8_t*)raw;
    o.pitch = (int64_t)W * H * 3 / 2;
    o.W = W, o.H = H, o.nv12 = layout == HV_YUV_NV12, o.chroma = chroma;
    const uint32_t wh = (uint32_t)W * (uint32_t)H;
    if (layout == HV_YUV_NV12) {
        o.u_off = wh, o.v_off = wh + 1, o.c_ld = W, o.c_step = 2;
    } else {
        o.u_off = layout == HV_YUV_I420 ? wh : wh + wh / 4;
        o.v_off = layout == HV_YUV_I420 ? wh + wh / 4 : wh;
        o.c_ld = W / 2, o.c_step = 1;
    }
    return o;
}

__device__ __forceinline__ float widen(uint16_t v) { return h2f(v); }
__device__ __forceinline__ float widen(uint32_t v) { return __uint_as_float(v); }

// the bytes of p[0 .. n); VEC: p is 16-byte aligned and n == 8
template <typename E, bool VEC>
__device__ __forceinline__ void load_run(const E* p, int n, int rescale, int (&q)[kRun]) {
    if constexpr (VEC) {
        if constexpr (sizeof(E) == 2) {
            const u32x4 w = *(const u32x4*)p;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                q[2 * i] = (int)quantise(h2f((uint16_t)(w[i] & 0xFFFFu)), rescale);
                q[2 * i + 1] = (int)quantise(h2f((uint16_t)(w[i] >> 16)), rescale);
            }
        } else {
            const u32x4 a = *(const u32x4*)p, b = *(const u32x4*)(p + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                q[i] = (int)quantise(__uint_as_float(a[i]), rescale);
                q[4 + i] = (int)quantise(__uint_as_float(b[i]), rescale);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRun; ++j) q[j] = j < n ? (int)quantise(widen(p[j]), rescale) : 0;
    }
}

__device__ __forceinline__ int luma(int R, int G, int B) {
    return (269484 * R + 528482 * G + 102760 * B + (16 << 20) + (1 << 19)) >> 20;
}
// S = 0: one pixel's bytes; S = 2: the sums of four
template <int S>
__device__ __forceinline__ int chroma_u(int R, int G, int B) {
    return (-155188 * R - 305135 * G + 460324 * B + (128 << (20 + S)) + (1 << (19 + S))) >> (20 + S);
}
template <int S>
__device__ __forceinline__ int chroma_v(int R, int G, int B) {
    return (460324 * R - 385875 * G - 74448 * B + (128 << (20 + S)) + (1 << (19 + S))) >> (20 + S);
}

__device__ __forceinline__ uint32_t pack4(const int* v) {
    return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

template <typename E, bool VEC>
__global__ __launch_bounds__(kThreads) void yuv_write_kernel(In in, Out o, int T) {
    const int W = o.W, cw = (W + kRun - 1) / kRun;
    const int units = (o.H / 2) * cw;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const E* xt = (const E*)in.x + (int64_t)t * in.st;
        uint8_t* f = o.raw + (int64_t)t * o.pitch;
        for (int u = blockIdx.x * kThreads + threadIdx.x; u < units; u += gridDim.x * kThreads) {
            const int r = u / cw, c = u - r * cw;
            const int x0 = c * kRun, n = min(kRun, W - x0);
            int q[2][3][kRun];
#pragma unroll
            for (int row = 0; row < 2; ++row) {
                const E* p = xt + (int64_t)(2 * r + row) * in.sh + x0;
                load_run<E, VEC>(p, n, in.rescale, q[row][0]);
                if (in.C == 3) {
                    load_run<E, VEC>(p + in.sc, n, in.rescale, q[row][1]);
                    load_run<E, VEC>(p + 2 * in.sc, n, in.rescale, q[row][2]);
                } else {
#pragma unroll
                    for (int j = 0; j < kRun; ++j) q[row][1][j] = q[row][2][j] = q[row][0][j];
                }
            }
            int Y[2][kRun], U[kRun / 2], V[kRun / 2];
#pragma unroll
            for (int row = 0; row < 2; ++row)
#pragma unroll
                for (int j = 0; j < kRun; ++j) Y[row][j] = luma(q[row][0][j], q[row][1][j], q[row][2][j]);
#pragma unroll
            for (int j = 0; j < kRun / 2; ++j) {
                const int a = 2 * j, b = 2 * j + 1;
                if (o.chroma) {
                    const int Rs = q[0][0][a] + q[0][0][b] + q[1][0][a] + q[1][0][b];
                    const int Gs = q[0][1][a] + q[0][1][b] + q[1][1][a] + q[1][1][b];
                    const int Bs = q[0][2][a] + q[0][2][b] + q[1][2][a] + q[1][2][b];
                    U[j] = chroma_u<2>(Rs, Gs, Bs), V[j] = chroma_v<2>(Rs, Gs, Bs);
                } else {
                    U[j] = chroma_u<0>(q[0][0][a], q[0][1][a], q[0][2][a]), V[j] = chroma_v<0>(q[0][0][a], q[0][1][a], q[0][2][a]);
                }
            }
            const uint32_t yo = (uint32_t)(2 * r) * W + x0;
            const uint32_t co = (uint32_t)r * o.c_ld + (uint32_t)(x0 >> 1) * o.c_step;
            if constexpr (VEC) {
                *(u32x2*)(f + yo) = u32x2{pack4(Y[0]), pack4(Y[0] + 4)};
                *(u32x2*)(f + yo + W) = u32x2{pack4(Y[1]), pack4(Y[1] + 4)};
                if (o.nv12) {                        // U0 V0 U1 V1 | U2 V2 U3 V3
                    const int lo[4] = {U[0], V[0], U[1], V[1]}, hi[4] = {U[2], V[2], U[3], V[3]};
                    *(u32x2*)(f + o.u_off + co) = u32x2{pack4(lo), pack4(hi)};
                } else {
                    *(uint32_t*)(f + o.u_off + co) = pack4(U);
                    *(uint32_t*)(f + o.v_off + co) = pack4(V);
                }
            } else {
#pragma unroll
                for (int j = 0; j < kRun; ++j)
                    if (j < n) {
                        f[yo + j] = (uint8_t)Y[0][j];
                        f[yo + W + j] = (uint8_t)Y[1][j];
                    }
#pragma unroll
                for (int j = 0; j < kRun / 2; ++j)
                    if (2 * j < n) {
                        f[o.u_off + co + j * o.c_step] = (uint8_t)U[j];
                        f[o.v_off + co + j * o.c_step] = (uint8_t)V[j];
                    }
            }
        }
    }
}

dim3 grid_for(int units, int T) {
    const int wgs = (units + kThreads - 1) / kThreads;
    const int gx = wgs < kMaxWgs ? wgs : kMaxWgs;
    const int gy = T < kMaxWgs / gx ? T : kMaxWgs / gx;     // kMaxWgs / gx >= 1
    return dim3((unsigned)gx, (unsigned)gy);
}

template <typename E>
int launch(const In& in, const Out& o, int T, hipStream_t stream) {
    const int q = 16 / (int)sizeof(E);
    const dim3 grid = grid_for((o.H / 2) * ((o.W + kRun - 1) / kRun), T);
    // W % 8 == 0 puts every Y row, chroma row and plane of every frame on an 8- (chroma planes: 4-) byte boundary of an aligned buffer,
    // and every run of an aligned input with aligned strides on a 16-byte boundary
    const bool vec = o.W % kRun == 0 && ((uintptr_t)o.raw & 7) == 0 && hv_aligned16(in.x) && in.st % q == 0 && in.sh % q == 0 &&
                     (in.C == 1 || in.sc % q == 0);
    if (vec)
        yuv_write_kernel<E, true><<<grid, dim3(kThreads), 0, stream>>>(in, o, T);
    else
        yuv_write_kernel<E, false><<<grid, dim3(kThreads), 0, stream>>>(in, o, T);
    return hv_check_launch();
}

}  // namespace

extern "C" int hv_clip_to_yuv420(const void* x, int dtype, int C, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, int rescale,
                                 int layout, int chroma, void* raw, hipStream_t stream) {
    if (!x || !raw || T < 1 || (dtype != 0 && dtype != 1) || (C != 1 && C != 3)) return HV_ERR_ARG;
    if ((rescale != 0 && rescale != 1) || (chroma != HV_YUVW_CHROMA_TOPLEFT && chroma != HV_YUVW_CHROMA_MEAN)) return HV_ERR_ARG;
    if (layout != HV_YUV_I420 && layout != HV_YUV_YV12 && layout != HV_YUV_NV12) return HV_ERR_ARG;
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || W > HV_YUV_MAX_SIDE || H > HV_YUV_MAX_SIDE) return HV_ERR_ARG;
    if (((uintptr_t)x & (dtype == 0 ? 1 : 3)) != 0) return HV_ERR_ARG;
    if (sc < 0 || st < 0 || sh < 0) return HV_ERR_ARG;
    const In in{x, sc, st, sh, C, rescale};
    const Out o = make_out(raw, layout, chroma, W, H);
    if (dtype == 0) return launch<uint16_t>(in, o, T, stream);
    return launch<uint32_t>(in, o, T, stream);
}
