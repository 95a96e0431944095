// Raw planar YUV 4:2:0 frames -> the clip tensor [3,T,OH,OW] in [-1, 1] the VAE and the scorers take (the fork's
// dataset_processor/yuv_tensor.py: cv2.cvtColor(COLOR_YUV2BGR_I420 / YV12 / NV12), COLOR_BGR2RGB, an optional cv2.resize, ToTensor and
// 2x - 1), in one pass: the 8-bit RGB frame never reaches memory.  Integer arithmetic and two table lookups, no floating point:
//
//   colour   BT.601 limited range in 20 fractional bits (OpenCV's fixed-point rule as restated in include/hv_kernels.h), pixel (y, x)
//            with the chroma sample (y >> 1, x >> 1);
//   resize   2-tap bilinear per axis on the 8-bit R, G, B, coefficients in HV_YUV_COEF_BITS (11) bits from the caller's axis tables:
//            h_r = c0x P[y_r][x0] + c1x P[y_r][x1],  out = (c0y h_0 + c1y h_1 + 2^21) >> 22;
//   value    vtab[q]: the caller's 256 entries in the output dtype (fp16 or fp32 bits).
//
//   yuv_copy_kernel<E, VEC>    OH == H, OW == W.  A thread owns 8 pixels of two adjacent rows, which share their four chroma samples: VEC
//                              loads 2 x 8 bytes of Y and 2 x 4 bytes (NV12: 8 bytes) of chroma and stores 16 bytes per lane per channel
//                              row (fp32: two of them); without VEC (W % 8 != 0: rows then start at odd 8-byte phases; or an unaligned
//                              source, output or stride) the same run is read byte by byte and written element by element.
//   yuv_resize_kernel<E>       a thread owns 8 output pixels of one row and gathers the four taps of each, every tap converted from its
//                              own Y, U, V bytes; neighbouring threads re-read the same source bytes through L2.
//
// Both are streaming kernels: grid.x strides over the units of a frame (at most 2048 workgroups over the whole grid), grid.y over the
// frames.  Frame and output offsets are 64-bit (a 1080p file passes 2^31 bytes at frame 691); offsets inside one source frame fit 32
// bits (W, H <= HV_YUV_MAX_SIDE).  No atomics; every output cell is written once.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWgs = 2048;
constexpr int kRun = 8;                      // pixels of one row a thread owns
constexpr int kCoefBits = HV_YUV_COEF_BITS;
constexpr int kCoefOne = 1 << kCoefBits;

struct Src {
    const uint8_t* raw;
    int64_t pitch;                           // bytes of one frame: W * H * 3 / 2
    int W, H, layout;
    uint32_t u_off, v_off;                   // first byte of U and V inside a frame (NV12: of the pair and of its second byte)
    int c_ld, c_step;                        // bytes between chroma rows, between chroma samples of one plane
};

struct Dst {
    void* out;
    int64_t sc, st, sh;
    int OH, OW;
};

__host__ Src make_src(const void* raw, int layout, int W, int H) {
    Src s;
    s.raw = (const uint8_t*)raw;
    s.pitch = (int64_t)W * H * 3 / 2;
    s.W = W, s.H = H, s.layout = layout;
    const uint32_t wh = (uint32_t)W * (uint32_t)H;
    if (layout == HV_YUV_NV12) {
        s.u_off = wh, s.v_off = wh + 1, s.c_ld = W, s.c_step = 2;
    } else {
        s.u_off = layout == HV_YUV_I420 ? wh : wh + wh / 4;
        s.v_off = layout == HV_YUV_I420 ? wh + wh / 4 : wh;
        s.c_ld = W / 2, s.c_step = 1;
    }
    return s;
}

__device__ __forceinline__ int clamp_byte(int v) { return min(max(v, 0), 255); }

// the chroma terms of one (U, V) sample, shared by the 2 x 2 pixels it covers
struct Chroma {
    int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(int U, int V) {
    const int u = U - 128, v = V - 128;
    return Chroma{1673527 * v, -852492 * v - 409993 * u, 2116026 * u};
}
__device__ __forceinline__ void yuv_to_rgb(int Y, const Chroma& c, int& R, int& G, int& B) {
    const int yy = max(0, Y - 16) * 1220542 + (1 << 19);
    R = clamp_byte((yy + c.r) >> 20);
    G = clamp_byte((yy + c.g) >> 20);
    B = clamp_byte((yy + c.b) >> 20);
}

template <typename E>
__device__ __forceinline__ void load_table(E* s_tab, const E* vtab) {
    for (int i = threadIdx.x; i < 256; i += kThreads) s_tab[i] = vtab[i];
    __syncthreads();
}

// v[0 .. n) to p; vec: p is 16-byte aligned and n == 8
template <typename E>
__device__ __forceinline__ void store_run(E* p, const E (&v)[kRun], int n, bool vec) {
    if (vec) {
        if constexpr (sizeof(E) == 2) {
            u32x4 w;
#pragma unroll
            for (int i = 0; i < 4; ++i) w[i] = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 16);
            *(u32x4*)p = w;
        } else {
            *(u32x4*)p = u32x4{v[0], v[1], v[2], v[3]};
            *(u32x4*)(p + 4) = u32x4{v[4], v[5], v[6], v[7]};
        }
    } else {
#pragma unroll
        for (int j = 0; j < kRun; ++j)
            if (j < n) p[j] = v[j];
    }
}

template <typename E, bool VEC>
__global__ __launch_bounds__(kThreads) void yuv_copy_kernel(Src s, Dst d, int T, const E* __restrict__ vtab) {
    __shared__ E s_tab[256];
    load_table(s_tab, vtab);
    const int W = s.W, cw = (W + kRun - 1) / kRun;
    const int units = (s.H / 2) * cw;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const uint8_t* f = s.raw + (int64_t)t * s.pitch;
        E* o = (E*)d.out + (int64_t)t * d.st;
        for (int u = blockIdx.x * kThreads + threadIdx.x; u < units; u += gridDim.x * kThreads) {
            const int r = u / cw, c = u - r * cw;
            const int x0 = c * kRun, n = min(kRun, W - x0);
            const uint32_t yo = (uint32_t)(2 * r) * W + x0;
            const uint32_t co = (uint32_t)r * s.c_ld + (uint32_t)(x0 >> 1) * s.c_step;
            int Y0[kRun], Y1[kRun], U[kRun / 2], V[kRun / 2];
            if constexpr (VEC) {
                const u32x2 a = *(const u32x2*)(f + yo), b = *(const u32x2*)(f + yo + W);
                uint32_t pu, pv;
                if (s.layout == HV_YUV_NV12) {       // U0 V0 U1 V1 | U2 V2 U3 V3
                    const u32x2 uv = *(const u32x2*)(f + s.u_off + co);
                    pu = (uv[0] & 0xFF) | ((uv[0] >> 8) & 0xFF00) | ((uv[1] & 0xFF) << 16) | ((uv[1] << 8) & 0xFF000000u);
                    pv = ((uv[0] >> 8) & 0xFF) | ((uv[0] >> 16) & 0xFF00) | ((uv[1] << 8) & 0xFF0000) | (uv[1] & 0xFF000000u);
                } else {
                    pu = *(const uint32_t*)(f + s.u_off + co);
                    pv = *(const uint32_t*)(f + s.v_off + co);
                }
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    Y0[j] = (a[j >> 2] >> (8 * (j & 3))) & 0xFF;
                    Y1[j] = (b[j >> 2] >> (8 * (j & 3))) & 0xFF;
                }
#pragma unroll
                for (int j = 0; j < kRun / 2; ++j) {
                    U[j] = (pu >> (8 * j)) & 0xFF;
                    V[j] = (pv >> (8 * j)) & 0xFF;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kRun; ++j) {
                    const bool ok = j < n;
                    Y0[j] = ok ? f[yo + j] : 0;
                    Y1[j] = ok ? f[yo + W + j] : 0;
                }
#pragma unroll
                for (int j = 0; j < kRun / 2; ++j) {
                    const bool ok = 2 * j < n;
                    U[j] = ok ? f[s.u_off + co + j * s.c_step] : 0;
                    V[j] = ok ? f[s.v_off + co + j * s.c_step] : 0;
                }
            }
            E v[2][3][kRun];
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                const Chroma ch = chroma_terms(U[j >> 1], V[j >> 1]);
                int R, G, B;
                yuv_to_rgb(Y0[j], ch, R, G, B);
                v[0][0][j] = s_tab[R], v[0][1][j] = s_tab[G], v[0][2][j] = s_tab[B];
                yuv_to_rgb(Y1[j], ch, R, G, B);
                v[1][0][j] = s_tab[R], v[1][1][j] = s_tab[G], v[1][2][j] = s_tab[B];
            }
#pragma unroll
            for (int row = 0; row < 2; ++row)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    store_run(o + k * d.sc + (int64_t)(2 * r + row) * d.sh + x0, v[row][k], n, VEC);
        }
    }
}

__device__ __forceinline__ void rgb_at(const uint8_t* f, const Src& s, int y, int x, int& R, int& G, int& B) {
    const uint32_t co = (uint32_t)(y >> 1) * s.c_ld + (uint32_t)(x >> 1) * s.c_step;
    yuv_to_rgb(f[(uint32_t)y * s.W + x], chroma_terms(f[s.u_off + co], f[s.v_off + co]), R, G, B);
}

template <typename E>
__global__ __launch_bounds__(kThreads) void yuv_resize_kernel(Src s, Dst d, int T, const int* __restrict__ ytab,
                                                             const int* __restrict__ xtab, const E* __restrict__ vtab, int vec_ok) {
    __shared__ E s_tab[256];
    load_table(s_tab, vtab);
    const int OW = d.OW, cw = (OW + kRun - 1) / kRun;
    const int units = d.OH * cw;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const uint8_t* f = s.raw + (int64_t)t * s.pitch;
        E* o = (E*)d.out + (int64_t)t * d.st;
        for (int u = blockIdx.x * kThreads + threadIdx.x; u < units; u += gridDim.x * kThreads) {
            const int oy = u / cw, c = u - oy * cw;
            const int x0 = c * kRun, n = min(kRun, OW - x0);
            // a table entry outside its range cannot send a load outside the frame
            const int ya = min(max(ytab[2 * oy], 0), s.H - 1), yb = min(ya + 1, s.H - 1);
            const int cy1 = min(max(ytab[2 * oy + 1], 0), kCoefOne), cy0 = kCoefOne - cy1;
            E v[3][kRun];
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                const int ox = min(x0 + j, OW - 1);
                const int xa = min(max(xtab[2 * ox], 0), s.W - 1), xb = min(xa + 1, s.W - 1);
                const int cx1 = min(max(xtab[2 * ox + 1], 0), kCoefOne), cx0 = kCoefOne - cx1;
                int p[4][3];
                rgb_at(f, s, ya, xa, p[0][0], p[0][1], p[0][2]);
                rgb_at(f, s, ya, xb, p[1][0], p[1][1], p[1][2]);
                rgb_at(f, s, yb, xa, p[2][0], p[2][1], p[2][2]);
                rgb_at(f, s, yb, xb, p[3][0], p[3][1], p[3][2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int h0 = cx0 * p[0][k] + cx1 * p[1][k], h1 = cx0 * p[2][k] + cx1 * p[3][k];
                    v[k][j] = s_tab[(cy0 * h0 + cy1 * h1 + (1 << (2 * kCoefBits - 1))) >> (2 * kCoefBits)];
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) store_run(o + k * d.sc + (int64_t)oy * d.sh + x0, v[k], n, vec_ok && n == kRun);
        }
    }
}

// c, t, h with extents (3, T, OH) over rows of OW contiguous elements: no two cells of the view may share an address
bool strides_disjoint(int64_t sc, int64_t st, int64_t sh, int T, int OH, int OW) {
    int64_t stride[3] = {sc, st, sh};
    int64_t extent[3] = {3, T, OH};
    for (int i = 0; i < 3; ++i)
        if (stride[i] < 0) return false;
    for (int i = 0; i < 3; ++i)              // by stride, ascending
        for (int j = i + 1; j < 3; ++j)
            if (stride[j] < stride[i]) {
                const int64_t a = stride[i], b = extent[i];
                stride[i] = stride[j], extent[i] = extent[j];
                stride[j] = a, extent[j] = b;
            }
    int64_t span = OW;                       // elements from the first to behind the last cell of the dimensions so far
    for (int i = 0; i < 3; ++i) {
        if (extent[i] == 1) continue;
        if (stride[i] < span) return false;
        if (stride[i] > (INT64_MAX - span) / (extent[i] - 1)) return false;
        span += (extent[i] - 1) * stride[i];
    }
    return true;
}

dim3 grid_for(int units, int T) {
    const int wgs = (units + kThreads - 1) / kThreads;
    const int gx = wgs < kMaxWgs ? wgs : kMaxWgs;
    const int gy = T < kMaxWgs / gx ? T : kMaxWgs / gx;     // kMaxWgs / gx >= 1
    return dim3((unsigned)gx, (unsigned)gy);
}

template <typename E>
int launch(const Src& s, const Dst& d, int T, const int* ytab, const int* xtab, const void* vtab, hipStream_t stream) {
    const int es = (int)sizeof(E), q = 16 / es;
    const bool out_vec = ((uintptr_t)d.out & 15) == 0 && d.sc % q == 0 && d.st % q == 0 && d.sh % q == 0;
    if (d.OH == s.H && d.OW == s.W) {
        const dim3 grid = grid_for((s.H / 2) * ((s.W + kRun - 1) / kRun), T);
        // W % 8 == 0 puts every Y row, chroma row and plane of every frame on an 8- (chroma planes: 4-) byte boundary of an aligned file
        if (s.W % kRun == 0 && ((uintptr_t)s.raw & 7) == 0 && out_vec)
            yuv_copy_kernel<E, true><<<grid, dim3(kThreads), 0, stream>>>(s, d, T, (const E*)vtab);
        else
            yuv_copy_kernel<E, false><<<grid, dim3(kThreads), 0, stream>>>(s, d, T, (const E*)vtab);
    } else {
        const dim3 grid = grid_for(d.OH * ((d.OW + kRun - 1) / kRun), T);
        yuv_resize_kernel<E><<<grid, dim3(kThreads), 0, stream>>>(s, d, T, ytab, xtab, (const E*)vtab, out_vec ? 1 : 0);
    }
    return hv_check_launch();
}

}  // namespace

extern "C" int hv_yuv420_to_clip(const void* raw, int T, int layout, int W, int H, void* out, int dtype, int64_t sc, int64_t st,
                                 int64_t sh, int OH, int OW, const int* ytab, const int* xtab, const void* vtab, hipStream_t stream) {
    if (!raw || !out || !vtab || T < 1 || (dtype != 0 && dtype != 1)) return HV_ERR_ARG;
    if (layout != HV_YUV_I420 && layout != HV_YUV_YV12 && layout != HV_YUV_NV12) return HV_ERR_ARG;
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || W > HV_YUV_MAX_SIDE || H > HV_YUV_MAX_SIDE) return HV_ERR_ARG;
    if (OH < 1 || OW < 1 || OH > HV_YUV_MAX_SIDE || OW > HV_YUV_MAX_SIDE) return HV_ERR_ARG;
    if ((OH != H || OW != W) && (!ytab || !xtab)) return HV_ERR_ARG;
    if (((uintptr_t)vtab & (dtype == 0 ? 1 : 3)) != 0 || ((uintptr_t)out & (dtype == 0 ? 1 : 3)) != 0) return HV_ERR_ARG;
    if (!strides_disjoint(sc, st, sh, T, OH, OW)) return HV_ERR_ARG;
    const Src s = make_src(raw, layout, W, H);
    const Dst d{out, sc, st, sh, OH, OW};
    if (dtype == 0) return launch<uint16_t>(s, d, T, ytab, xtab, vtab, stream);
    return launch<uint32_t>(s, d, T, ytab, xtab, vtab, stream);
}
