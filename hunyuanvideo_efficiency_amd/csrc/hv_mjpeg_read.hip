// Baseline JPEG frames -> video tensor [3,T,H,W] (fp16 / fp32): the three stages of include/hv_mjpeg_read.h.
//
//   restarts_kernel      a workgroup per frame (grid-striding).  The frame's entropy-coded bytes are walked in strips of kThreads x
//                        kChunk bytes; a thread counts the RSTm markers that begin in its chunk, a workgroup prefix count numbers them in
//                        address order, and marker j < ipf - 1 ends interval j and begins interval j + 1.  No global atomics.
//   decode_kernel        one serial Huffman decoder per restart interval (csrc/hv_mjpeg_decode.hpp, the text the host fuzz program
//                        compiles), kDecoders of them in a one-wave workgroup: few lanes per wave keep the cost of divergent symbols
//                        low and spread the intervals of a clip over all CUs.  The four lookup tables are built in LDS from the
//                        tables in the argument block; a lane assembles each block in LDS and stores it whole (8 x 16 bytes), so
//                        every block of the interval is written exactly once, zeros where the stream stops.
//   clip_kernel          a workgroup per tile of 4 x 2 MCUs (64 x 32 pixels).  The tile's Y blocks and the chroma blocks of the tile
//                        and of one block around it (the triangle filter reads one sample across every tile edge) are dequantised
//                        and inverse-transformed into bytes in LDS: a thread per block column, then a thread per block row.  A thread
//                        per pixel then filters the chroma, converts to R, G, B and stores vtab[byte].  The filtered planes exist
//                        only in registers.
#include "hv_common.hpp"
#include "hv_mjpeg_decode.hpp"
#include "hv_wg_scan.hpp"
#include "../../include/hv_kernels.h"
#include "../../include/hv_mjpeg_read.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWgs = 4096;
constexpr int kChunk = 16;                                     // bytes a thread scans per strip
constexpr int kDecoders = 16;                                  // decoding lanes of a workgroup
constexpr int kDecThreads = 64;                                // one wave; also fills s_nat, a thread per entry
constexpr int kStageLd = 72;                                   // int16 per lane: 144 bytes keep every lane's block 16-byte aligned
constexpr int kTileX = 4, kTileY = 2;                          // MCUs of a tile
constexpr int kYBlocks = kTileX * kTileY * 4;                  // 32
constexpr int kCBx = kTileX + 2, kCBy = kTileY + 2;            // chroma blocks of a tile with its border
constexpr int kCBlocks = kCBx * kCBy;                          // 24 per component
constexpr int kBlocks = kYBlocks + 2 * kCBlocks;               // 80
constexpr int kYLd = kTileX * 16, kCLd = kCBx * 8;
constexpr int kWsLd = 65;                                      // int32 per block between the passes: blocks fall on different banks

static_assert(kThreads == kWgScanThreads, "wg_scan_excl (csrc/hv_wg_scan.hpp) sums over kThreads");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

struct RstArgs {
    const uint8_t* data;
    int64_t data_bytes;
    const int64_t *scan_begin, *scan_end;
    int T, ipf;
    int64_t *interval_begin, *interval_end;
    int32_t* found;
};

__global__ __launch_bounds__(kThreads) void restarts_kernel(RstArgs a) {
    __shared__ int s_scan[kThreads], s_bad;
    const int tid = threadIdx.x;
    for (int t = blockIdx.x; t < a.T; t += gridDim.x) {
        const int64_t begin = clamp64(a.scan_begin[t], 0, a.data_bytes);
        const int64_t end = clamp64(a.scan_end[t], begin, a.data_bytes);
        int64_t* ib = a.interval_begin + (int64_t)t * a.ipf;
        int64_t* ie = a.interval_end + (int64_t)t * a.ipf;
        if (tid == 0) s_bad = 0;
        __syncthreads();
        int64_t seen = 0;                                      // markers of the strips before this one
        for (int64_t s0 = begin; s0 < end; s0 += (int64_t)kThreads * kChunk) {
            const int64_t j0 = s0 + (int64_t)tid * kChunk;
            const int64_t j1 = j0 + kChunk < end - 1 ? j0 + kChunk : end - 1;      // a marker begins at j < end - 1
            int n = 0;
            for (int64_t j = j0; j < j1; ++j) n += a.data[j] == 0xFF && (a.data[j + 1] & 0xF8) == 0xD0;
            int total;
            int64_t k = seen + wg_scan_excl(n, s_scan, tid, total);
            if (n)
                for (int64_t j = j0; j < j1; ++j)
                    if (a.data[j] == 0xFF && (a.data[j + 1] & 0xF8) == 0xD0) {
                        if (k < a.ipf - 1) {
                            ie[k] = j;
                            ib[k + 1] = j + 2;
                            if ((a.data[j + 1] & 7) != (int)(k & 7)) s_bad = 1;
                        }
                        ++k;
                    }
            seen += total;
        }
        __syncthreads();
        const int64_t have = seen < a.ipf - 1 ? seen : a.ipf - 1;
        for (int64_t k = have + tid; k < a.ipf - 1; k += kThreads) ie[k] = end, ib[k + 1] = end;
        if (tid == 0) {
            ib[0] = begin;
            ie[a.ipf - 1] = end;
            a.found[t] = (int32_t)(seen < HV_MJPEG_RST_ORDER - 1 ? seen : HV_MJPEG_RST_ORDER - 1) | (s_bad ? HV_MJPEG_RST_ORDER : 0);
        }
        __syncthreads();
    }
}

struct HuffBytes {
    uint8_t t[HV_MJPEG_HUFF_BYTES];
};

struct DecArgs {
    const uint8_t* data;
    int64_t data_bytes;
    const int64_t *interval_begin, *interval_end;
    int Ri, ipf;
    int64_t mpf, units;
    int16_t* coefs;
    int32_t* status;
    HuffBytes huff;
};

__global__ __launch_bounds__(kDecThreads) void decode_kernel(DecArgs a) {
    __shared__ HvHuffTab s_tab[4];
    __shared__ __attribute__((aligned(16))) int16_t s_stage[kDecoders * kStageLd];
    __shared__ uint8_t s_nat[64];
    const int tid = threadIdx.x;
    if (tid < 4) hv_mjd_build(a.huff.t + tid * kMjdTableBytes, &s_tab[tid]);
    s_nat[tid] = (uint8_t)hv_mjd_natural(tid);
    __syncthreads();
    if (tid >= kDecoders) return;
    for (int64_t u = (int64_t)blockIdx.x * kDecoders + tid; u < a.units; u += (int64_t)gridDim.x * kDecoders) {
        const int64_t t = u / a.ipf, k = u - t * a.ipf;
        const int64_t m0 = k * a.Ri;                                                   // Ri = 0: ipf = 1, k = 0
        const int64_t n = a.Ri == 0 || a.mpf - m0 < a.Ri ? a.mpf - m0 : a.Ri;
        const int64_t begin = clamp64(a.interval_begin[u], 0, a.data_bytes);
        const int64_t end = clamp64(a.interval_end[u], begin, a.data_bytes);
        const int expect = k < a.ipf - 1 ? 0xD0 + (int)(k & 7) : 0;
        a.status[u] = hv_mjd_interval(a.data, begin, end, expect, s_tab, s_nat, n, s_stage + tid * kStageLd, a.coefs + (t * a.mpf + m0) * 384);
    }
}

struct QuantBytes {
    uint8_t q[HV_MJPEG_QUANT_BYTES];
};

struct ClipArgs {
    const int16_t* coefs;
    const void* vtab;
    void* out;
    int64_t sc, st, sh;
    int H, W, mcus, rows, tiles_x, tiles_y;
    QuantBytes quant;
};

// the 1-D pass of include/hv_mjpeg_read.h on d[0 .. 7] -> y[0 .. 7], unscaled.  The arithmetic is uint32 (the same bits as int32 while
// nothing overflows, i.e. for every stream an 8-bit coder produces, and a defined wrap modulo 2^32 for any other).
__device__ __forceinline__ void idct8(const int (&di)[8], int (&y)[8]) {
    uint32_t d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = (uint32_t)di[i];
    uint32_t z1 = (d[2] + d[6]) * 4433u;
    const uint32_t t2 = z1 - d[6] * 15137u, t3 = z1 + d[2] * 6270u;
    const uint32_t t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const uint32_t e0 = t0 + t3, e3 = t0 - t3, e1 = t1 + t2, e2 = t1 - t2;
    z1 = d[7] + d[1];
    uint32_t z2 = d[5] + d[3], z3 = d[7] + d[3], z4 = d[5] + d[1];
    const uint32_t z5 = (z3 + z4) * 9633u;
    uint32_t o0 = d[7] * 2446u, o1 = d[5] * 16819u, o2 = d[3] * 25172u, o3 = d[1] * 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995, z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
    o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
    y[0] = (int)(e0 + o3), y[7] = (int)(e0 - o3), y[1] = (int)(e1 + o2), y[6] = (int)(e1 - o2);
    y[2] = (int)(e2 + o1), y[5] = (int)(e2 - o1), y[3] = (int)(e3 + o0), y[4] = (int)(e3 - o0);
}

// (v + round) >> shift with the sum taken modulo 2^32, the shift arithmetic
__device__ __forceinline__ int descale(int v, uint32_t round, int shift) { return (int)((uint32_t)v + round) >> shift; }

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

template <typename E>
__global__ __launch_bounds__(kThreads) void clip_kernel(ClipArgs a) {
    __shared__ int s_ws[kBlocks * kWsLd];
    __shared__ uint8_t s_y[kTileY * 16 * kYLd], s_c[2][kCBy * 8 * kCLd];
    __shared__ int s_q[2][64];
    __shared__ E s_vtab[256];
    const int tid = threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int64_t per_frame = (int64_t)a.tiles_x * a.tiles_y;
    const int64_t t = tile / per_frame;
    const int ty = (int)((tile - t * per_frame) / a.tiles_x), tx = (int)(tile - t * per_frame - (int64_t)ty * a.tiles_x);
    const int mx0 = tx * kTileX, my0 = ty * kTileY;            // the tile's first MCU
    if (tid < 128) s_q[tid >> 6][tid & 63] = a.quant.q[tid];
    s_vtab[tid] = ((const E*)a.vtab)[tid];
    __syncthreads();

    // the workspace block of local block b: Y blocks first (MCU-major, 4 per MCU), then Cb and Cr of the bordered chroma grid; nullptr
    // for a block outside the frame's MCU grid (never read below: the filter clamps to the real chroma plane)
    auto block_src = [&](int b) -> const int16_t* {
        int mx, my, k;
        if (b < kYBlocks) {
            mx = mx0 + (b >> 2) % kTileX, my = my0 + (b >> 2) / kTileX, k = b & 3;
        } else {
            const int c = (b - kYBlocks) / kCBlocks, i = (b - kYBlocks) % kCBlocks;
            mx = mx0 - 1 + i % kCBx, my = my0 - 1 + i / kCBx, k = 4 + c;
        }
        if (mx < 0 || my < 0 || mx >= a.mcus || my >= a.rows) return nullptr;
        return a.coefs + ((t * a.rows + my) * a.mcus + mx) * 384 + k * 64;
    };
    // 1. columns: dequantise, first pass, (y + 2^10) >> 11
    for (int i = tid; i < kBlocks * 8; i += kThreads) {
        const int b = i >> 3, x = i & 7;
        const int16_t* src = block_src(b);
        if (!src) continue;
        const int* q = s_q[b >= kYBlocks];
        int d[8], y[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = (int)src[r * 8 + x] * q[r * 8 + x];
        idct8(d, y);
#pragma unroll
        for (int r = 0; r < 8; ++r) s_ws[b * kWsLd + r * 8 + x] = descale(y[r], 1024u, 11);
    }
    __syncthreads();
    // 2. rows: second pass, ((y + 2^17) >> 18) + 128, clamped -> the byte planes
    for (int i = tid; i < kBlocks * 8; i += kThreads) {
        const int b = i >> 3, r = i & 7;
        if (!block_src(b)) continue;
        int d[8], y[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) d[x] = s_ws[b * kWsLd + r * 8 + x];
        idct8(d, y);
        uint8_t* dst;
        if (b < kYBlocks) {
            const int m = b >> 2, k = b & 3;
            dst = s_y + ((m / kTileX) * 16 + (k >> 1) * 8 + r) * kYLd + (m % kTileX) * 16 + (k & 1) * 8;
        } else {
            const int c = (b - kYBlocks) / kCBlocks, j = (b - kYBlocks) % kCBlocks;
            dst = s_c[c] + ((j / kCBx) * 8 + r) * kCLd + (j % kCBx) * 8;
        }
#pragma unroll
        for (int x = 0; x < 8; ++x) dst[x] = (uint8_t)clamp255(descale(y[x], 1u << 17, 18) + 128);
    }
    __syncthreads();
    // 3. a thread per pixel: chroma filter, colour, value table
    const int ch = (a.H + 1) >> 1, cw = (a.W + 1) >> 1;
    const int px0 = mx0 * 16, py0 = my0 * 16;
    const int cx0 = mx0 * 8 - 8, cy0 = my0 * 8 - 8;            // chroma coordinates of s_c[.][0][0]
    E* const o = (E*)a.out + t * a.st;
    for (int i = tid; i < kTileY * 16 * kYLd; i += kThreads) {
        const int ly = i / kYLd, lx = i - ly * kYLd;
        const int py = py0 + ly, px = px0 + lx;
        if (py >= a.H || px >= a.W) continue;
        const int Y = s_y[ly * kYLd + lx];
        const int cy = py >> 1, cx = px >> 1;
        int cc[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint8_t* p = s_c[c];
            if (cw <= 2) {
                cc[c] = p[(cy - cy0) * kCLd + cx - cx0];
            } else {
                const int ry = (py & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                const int rx = (px & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
                const int s_here = 3 * p[(cy - cy0) * kCLd + cx - cx0] + p[(ry - cy0) * kCLd + cx - cx0];
                const int s_next = 3 * p[(cy - cy0) * kCLd + rx - cx0] + p[(ry - cy0) * kCLd + rx - cx0];
                cc[c] = (3 * s_here + s_next + ((px & 1) ? 7 : 8)) >> 4;
            }
        }
        const int cb = cc[0] - 128, cr = cc[1] - 128;
        const int R = clamp255(Y + ((91881 * cr + 32768) >> 16));
        const int G = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        const int B = clamp255(Y + ((116130 * cb + 32768) >> 16));
        E* const dst = o + (int64_t)py * a.sh + px;
        dst[0] = s_vtab[R];
        dst[a.sc] = s_vtab[G];
        dst[2 * a.sc] = s_vtab[B];
    }
}

// c, t, h with extents (3, T, H) over rows of W contiguous elements: no two cells of the view may share an address (hv_yuv.hip's rule)
bool strides_disjoint(int64_t sc, int64_t st, int64_t sh, int T, int H, int W) {
    int64_t stride[3] = {sc, st, sh};
    int64_t extent[3] = {3, T, H};
    for (int i = 0; i < 3; ++i)
        if (stride[i] < 0) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (stride[j] < stride[i]) {
                const int64_t s = stride[i], e = extent[i];
                stride[i] = stride[j], extent[i] = extent[j];
                stride[j] = s, extent[j] = e;
            }
    int64_t span = W;
    for (int i = 0; i < 3; ++i) {
        if (extent[i] == 1) continue;
        if (stride[i] < span) return false;
        if (stride[i] > (INT64_MAX - span) / (extent[i] - 1)) return false;
        span += (extent[i] - 1) * stride[i];
    }
    return true;
}

bool shape_ok(int T, int H, int W) { return T >= 1 && H >= 1 && W >= 1 && H <= HV_YUV_MAX_SIDE && W <= HV_YUV_MAX_SIDE; }
int64_t mcus_per_frame(int H, int W) { return (int64_t)((W + 15) / 16) * ((H + 15) / 16); }

}  // namespace

extern "C" int64_t hv_mjpeg_coef_bytes(int T, int H, int W) {
    if (!shape_ok(T, H, W)) return 0;
    return (int64_t)T * mcus_per_frame(H, W) * HV_MJPEG_COEF_BYTES_PER_MCU;
}

extern "C" int hv_mjpeg_find_restarts(const void* data, int64_t data_bytes, const int64_t* scan_begin, const int64_t* scan_end, int T,
                                      int ipf, int64_t* interval_begin, int64_t* interval_end, int32_t* found, hipStream_t stream) {
    if (!data || !scan_begin || !scan_end || !interval_begin || !interval_end || !found) return HV_ERR_ARG;
    if (T < 1 || ipf < 1 || data_bytes < 0 || (int64_t)T * ipf > 0x7fffffff) return HV_ERR_ARG;
    if ((((uintptr_t)scan_begin | (uintptr_t)scan_end | (uintptr_t)interval_begin | (uintptr_t)interval_end) & 7) != 0) return HV_ERR_ARG;
    if (((uintptr_t)found & 3) != 0) return HV_ERR_ARG;
    const RstArgs a{(const uint8_t*)data, data_bytes, scan_begin, scan_end, T, ipf, interval_begin, interval_end, found};
    restarts_kernel<<<dim3((unsigned)(T < kMaxWgs ? T : kMaxWgs)), dim3(kThreads), 0, stream>>>(a);
    return hv_check_launch();
}

extern "C" int hv_mjpeg_decode_coefs(const void* data, int64_t data_bytes, const int64_t* interval_begin, const int64_t* interval_end,
                                     int T, int H, int W, int Ri, int ipf, const uint8_t* huff_tables, void* coefs, int64_t coef_bytes,
                                     int32_t* status, hipStream_t stream) {
    if (!data || !interval_begin || !interval_end || !huff_tables || !coefs || !status) return HV_ERR_ARG;
    if (!shape_ok(T, H, W) || data_bytes < 0 || Ri < 0) return HV_ERR_ARG;
    const int64_t mpf = mcus_per_frame(H, W);
    if (ipf != (Ri == 0 ? 1 : (mpf + Ri - 1) / Ri) || (int64_t)T * ipf > 0x7fffffff) return HV_ERR_ARG;
    if (coef_bytes < hv_mjpeg_coef_bytes(T, H, W) || ((uintptr_t)coefs & 15) != 0) return HV_ERR_ARG;
    if ((((uintptr_t)interval_begin | (uintptr_t)interval_end) & 7) != 0 || ((uintptr_t)status & 3) != 0) return HV_ERR_ARG;
    if (!hv_mjd_tables_ok(huff_tables)) return HV_ERR_ARG;
    DecArgs a{(const uint8_t*)data, data_bytes, interval_begin, interval_end, Ri, ipf, mpf, (int64_t)T * ipf, (int16_t*)coefs, status, {}};
    for (int i = 0; i < HV_MJPEG_HUFF_BYTES; ++i) a.huff.t[i] = huff_tables[i];
    const int64_t wgs = (a.units + kDecoders - 1) / kDecoders;
    decode_kernel<<<dim3((unsigned)(wgs < kMaxWgs ? wgs : kMaxWgs)), dim3(kDecThreads), 0, stream>>>(a);
    return hv_check_launch();
}

extern "C" int hv_mjpeg_coefs_to_clip(const void* coefs, int64_t coef_bytes, const uint8_t* quant_tables, const void* vtab, void* out,
                                      int dtype, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, hipStream_t stream) {
    if (!coefs || !quant_tables || !vtab || !out || (dtype != 0 && dtype != 1)) return HV_ERR_ARG;
    if (!shape_ok(T, H, W)) return HV_ERR_ARG;
    if (coef_bytes < hv_mjpeg_coef_bytes(T, H, W) || ((uintptr_t)coefs & 15) != 0) return HV_ERR_ARG;
    if ((((uintptr_t)vtab | (uintptr_t)out) & (dtype == 0 ? 1 : 3)) != 0) return HV_ERR_ARG;
    if (!strides_disjoint(sc, st, sh, T, H, W)) return HV_ERR_ARG;
    ClipArgs a{(const int16_t*)coefs, vtab, out, sc, st, sh, H, W, (W + 15) / 16, (H + 15) / 16, 0, 0, {}};
    for (int i = 0; i < HV_MJPEG_QUANT_BYTES; ++i) {
        if (quant_tables[i] == 0) return HV_ERR_ARG;
        a.quant.q[i] = quant_tables[i];
    }
    a.tiles_x = (a.mcus + kTileX - 1) / kTileX, a.tiles_y = (a.rows + kTileY - 1) / kTileY;
    const int64_t tiles = (int64_t)T * a.tiles_x * a.tiles_y;
    if (!hv_grid_x_ok(tiles)) return HV_ERR_ARG;
    if (dtype == 0)
        clip_kernel<uint16_t><<<dim3((unsigned)tiles), dim3(kThreads), 0, stream>>>(a);
    else
        clip_kernel<uint32_t><<<dim3((unsigned)tiles), dim3(kThreads), 0, stream>>>(a);
    return hv_check_launch();
}
