// Video tensor [C,T,H,W] (fp16 / fp32) -> the entropy-coded data of baseline JPEG frames (ITU-T T.81), one restart interval per MCU row.
// The rule is stated in include/hv_mjpeg.h: the quantiser of the scoring kernels (hv_common.hpp: quantise), JFIF BT.601 in 16 fractional
// bits, 4:2:0 chroma from 2 x 2 sums, an integer 8 x 8 DCT, Annex K quantisation tables under the IJG quality rule, the four Annex K
// Huffman tables.  Everything behind the quantiser is integer arithmetic: tests/mjpeg_ref.py restates it byte for byte.
//
//   mjpeg_kernel<E, WRITE>   one workgroup per unit (frame, MCU row), grid-striding over the units (at most kMaxWgs workgroups).  A row
//                            is coded in passes of kPassMcus MCUs (96 blocks), so LDS holds a pass, never a row, and a row of any legal
//                            width (1024 MCUs) is a loop.  A pass:
//                              1. a thread per 2 x 2 pixels: quantise, Y per pixel, Cb / Cr of the sums -> LDS bytes (edges replicated);
//                              2. a thread per block row: the row pass of the DCT -> t1 (int16) in LDS;
//                              3. a thread per block column: the column pass, quantisation -> coefficients in zigzag order (int16, LDS);
//                              4. a thread per block: the length of its code bits; a workgroup prefix sum gives every block its bit offset;
//                              5. a thread per block: the bits again, OR-ed (LDS atomics) into a zeroed bit buffer sized for the worst
//                                 case of a pass (96 blocks x 1660 bits = 19.9 KB), so no content can overflow it;
//                              6. the pass's whole bytes: a thread per contiguous chunk counts its 0xFF bytes, a second prefix sum gives
//                                 the chunk's place behind the stuffing, and (WRITE) the chunk is stored with its 0x00 bytes.
//                            The 0 .. 7 bits behind the last whole byte go to the next pass as its first bits; the last pass pads them
//                            with 1-bits.  DC predictors cross passes in LDS.  WRITE = false only counts (hv_mjpeg_measure), WRITE = true
//                            stores at offsets[u] (hv_mjpeg_write): both derive the coefficients from the pixels, there is no workspace.
//
// The pixel and t1 staging of steps 1 - 3 and the bit buffer of steps 5 - 6 share one LDS region (36 KB a workgroup in all).  Offsets into
// `scan` are 64-bit; no store lands at or past offsets[u + 1]; no global atomics; every byte is written once, by plain byte stores.
#include "hv_common.hpp"
#include "../../include/hv_kernels.h"
#include "../../include/hv_mjpeg.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWgs = 2048;
constexpr int kPassMcus = 16;                                  // MCUs of one pass
constexpr int kPassBlocks = kPassMcus * 6;                     // Y00 Y01 Y10 Y11 Cb Cr
constexpr int kCoefLd = 66;                                    // int16 per block in LDS: 33 words, blocks fall on different banks
constexpr int kBlockBitsMax = 22 + 63 * 26;                    // DC: 11-bit code + 11 bits; an AC coefficient: 16-bit code + 10 bits
constexpr int kBitWords = (7 + kPassBlocks * kBlockBitsMax + 31) / 32 + 1;
constexpr int kYLd = kPassMcus * 16;                           // bytes of a Y row of a pass
constexpr int kCLd = kPassMcus * 8;
constexpr int kStageBytes = 16 * kYLd + 2 * 8 * kCLd + kPassBlocks * kCoefLd * 2;
static_assert(kStageBytes <= kBitWords * 4, "the staging of steps 1 - 3 lives inside the bit buffer");
static_assert(kPassBlocks <= kThreads, "steps 4 and 5 give every block of a pass its own thread");

// M[u][x] = round(8192 a(u) cos((2x + 1) u pi / 16))
constexpr int kM[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},   {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                          {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                          {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                          {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};

// T.81 Annex K.1, K.2 in natural order
__device__ const uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// zigzag position of every natural index (T.81 Figure A.6)
__device__ const uint8_t kZigOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43,
                                       9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                       21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
// T.81 Annex K.3 - K.6: BITS of DC luminance, AC luminance, DC chrominance, AC chrominance; HUFFVAL (both DC tables: 0 .. 11)
__device__ const uint8_t kHuffBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125},
                                             {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
__device__ const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
     0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
     0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
     0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
     0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
     0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
     0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
     0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};

struct Args {
    const void* x;
    int64_t sc, st, sh;
    int C, rescale, H, W, quality;
    int mcus, rows;                          // MCUs of a row, MCU rows of a frame
    int64_t units;                           // T * rows
    int32_t* sizes;                          // measure: interval_bytes
    const int64_t* offsets;                  // write
    uint8_t* scan;
};

__device__ __forceinline__ float widen(uint16_t v) { return h2f(v); }
__device__ __forceinline__ float widen(uint32_t v) { return __uint_as_float(v); }

// T.81 Annex C: symbol -> (length << 16) | code
__device__ void build_huff(const uint8_t* bits, const uint8_t* vals, uint32_t* tab) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i) tab[vals ? vals[k++] : k++] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
}

// exclusive prefix sum of v over the workgroup; total = the sum.  s: kThreads ints of LDS, free again on return.
__device__ int wg_scan_excl(int v, int* s, int tid, int& total) {
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int a = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    total = s[kThreads - 1];
    const int ex = s[tid] - v;
    __syncthreads();
    return ex;
}

// the code bits of a block, most significant first, OR-ed into 32-bit words of LDS (bit 31 of word 0 is the first bit of the buffer)
struct Sink {
    uint32_t* words;
    uint64_t acc;                            // the low n bits are pending
    int n, w;
    __device__ __forceinline__ void put(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            atomicOr(&words[w++], (uint32_t)(acc >> (n - 32)));
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(&words[w], (uint32_t)(acc << (32 - n)));
    }
};

// T.81 F.1.2: the DC difference and the AC coefficients of one block in zigzag order; returns the number of bits
template <bool EMIT>
__device__ int code_block(const int16_t* c, int pred, const uint32_t* dc, const uint32_t* ac, Sink& s) {
    int bits = 0;
    auto put = [&](uint32_t entry, int v, int cat) {
        const int len = (int)(entry >> 16) + cat;
        if constexpr (EMIT) s.put(((entry & 0xFFFFu) << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u)), len);
        bits += len;
    };
    const int d = (int)c[0] - pred;
    put(dc[d ? 32 - __clz(abs(d)) : 0], d, d ? 32 - __clz(abs(d)) : 0);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) put(ac[0xF0], 0, 0);                       // ZRL
        const int cat = 32 - __clz(abs(v));
        put(ac[(run << 4) | cat], v, cat);
        run = 0;
    }
    if (run > 0) put(ac[0x00], 0, 0);                                            // EOB
    return bits;
}

template <typename E, bool WRITE>
__global__ __launch_bounds__(kThreads) void mjpeg_kernel(Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_bits[kBitWords];
    __shared__ int16_t s_coef[kPassBlocks * kCoefLd];
    __shared__ uint32_t s_ac[2][256], s_dc[2][16];
    __shared__ int s_q[2][64], s_scan[kThreads], s_lastdc[3], s_carry[2];
    __shared__ uint8_t s_zig[64];
    uint8_t* const s_y = (uint8_t*)s_bits;                    // [16][kYLd]
    uint8_t* const s_c = s_y + 16 * kYLd;                     // [2][8][kCLd]
    int16_t* const s_t1 = (int16_t*)(s_c + 2 * 8 * kCLd);     // [kPassBlocks][kCoefLd]
    const int tid = threadIdx.x;

    for (int i = tid; i < 512; i += kThreads) (&s_ac[0][0])[i] = 0;
    if (tid < 32) (&s_dc[0][0])[tid] = 0;
    if (tid < 64) s_zig[tid] = kZigOf[tid];
    if (tid < 128) {
        const int s = a.quality < 50 ? 5000 / a.quality : 200 - 2 * a.quality;
        const int q = ((int)kBaseQ[tid >> 6][tid & 63] * s + 50) / 100;
        s_q[tid >> 6][tid & 63] = min(max(q, 1), 255);
    }
    __syncthreads();
    if (tid == 0) build_huff(kHuffBits[0], nullptr, s_dc[0]);
    if (tid == 64) build_huff(kHuffBits[1], kAcVals[0], s_ac[0]);
    if (tid == 128) build_huff(kHuffBits[2], nullptr, s_dc[1]);
    if (tid == 192) build_huff(kHuffBits[3], kAcVals[1], s_ac[1]);
    __syncthreads();

    const int W = a.W, H = a.H;
    for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int64_t t = u / a.rows;
        const int row = (int)(u - t * a.rows);
        const E* xt = (const E*)a.x + t * a.st;
        uint8_t* dst = nullptr;
        int64_t limit = 0, out_run = 0;                        // bytes of this interval: allowed (WRITE), produced so far
        if constexpr (WRITE) {
            dst = a.scan + a.offsets[u];
            limit = a.offsets[u + 1] - a.offsets[u];
        }
        if (tid < 3) s_lastdc[tid] = 0;
        if (tid < 2) s_carry[tid] = 0;                         // [0]: 0 .. 7 bits left over by the previous pass, [1]: their value
        __syncthreads();

        for (int m0 = 0; m0 < a.mcus; m0 += kPassMcus) {
            const int nm = min(kPassMcus, a.mcus - m0), nb = nm * 6;
            const bool last = m0 + kPassMcus >= a.mcus;
            // 1. pixels -> bytes -> Y, and Cb / Cr of every 2 x 2 block
            const int qw = nm * 8;
            for (int i = tid; i < qw * 8; i += kThreads) {
                const int qy = i / qw, qx = i - qy * qw;
                int rs = 0, gs = 0, bs = 0;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int py = min(row * 16 + qy * 2 + dy, H - 1), px = min(m0 * 16 + qx * 2 + dx, W - 1);
                        const E* p = xt + (int64_t)py * a.sh + px;
                        const int r = (int)quantise(widen(p[0]), a.rescale);
                        int g = r, b = r;
                        if (a.C == 3) {
                            g = (int)quantise(widen(p[a.sc]), a.rescale);
                            b = (int)quantise(widen(p[2 * a.sc]), a.rescale);
                        }
                        s_y[(qy * 2 + dy) * kYLd + qx * 2 + dx] = (uint8_t)min(max((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0), 255);
                        rs += r, gs += g, bs += b;
                    }
                const int cb = (-11059 * rs - 21709 * gs + 32768 * bs + (128 << 18) + (1 << 17)) >> 18;
                const int cr = (32768 * rs - 27439 * gs - 5329 * bs + (128 << 18) + (1 << 17)) >> 18;
                s_c[qy * kCLd + qx] = (uint8_t)min(max(cb, 0), 255);
                s_c[8 * kCLd + qy * kCLd + qx] = (uint8_t)min(max(cr, 0), 255);
            }
            __syncthreads();
            // 2. row pass: t[y][u] = sum_x M[u][x] s[y][x], t1 = (t + 128) >> 8
            for (int i = tid; i < nb * 8; i += kThreads) {
                const int b = i >> 3, y = i & 7, mcu = b / 6, k = b - mcu * 6;
                const uint8_t* src = k < 4 ? s_y + ((k >> 1) * 8 + y) * kYLd + mcu * 16 + (k & 1) * 8 : s_c + (k - 4) * 8 * kCLd + y * kCLd + mcu * 8;
                const u32x2 w = *(const u32x2*)src;
                int s[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) s[x] = (int)((w[x >> 2] >> (8 * (x & 3))) & 0xFFu) - 128;
#pragma unroll
                for (int uu = 0; uu < 8; ++uu) {
                    int acc = 0;
#pragma unroll
                    for (int x = 0; x < 8; ++x) acc += kM[uu][x] * s[x];
                    s_t1[b * kCoefLd + y * 8 + uu] = (int16_t)((acc + 128) >> 8);
                }
            }
            __syncthreads();
            // 3. column pass r[v][u] = sum_y M[v][y] t1[y][u], quantised, stored in zigzag order
            for (int i = tid; i < nb * 8; i += kThreads) {
                const int b = i >> 3, uu = i & 7, comp = (b % 6) >= 4;
                int c[8];
#pragma unroll
                for (int y = 0; y < 8; ++y) c[y] = s_t1[b * kCoefLd + y * 8 + uu];
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    int r = 0;
#pragma unroll
                    for (int y = 0; y < 8; ++y) r += kM[v][y] * c[y];
                    const uint32_t Q = (uint32_t)s_q[comp][v * 8 + uu];
                    const int q = (int)(((uint32_t)abs(r) + (Q << 17)) / (Q << 18));
                    s_coef[b * kCoefLd + s_zig[v * 8 + uu]] = (int16_t)(r < 0 ? -q : q);
                }
            }
            __syncthreads();
            // 4. bits of every block, their prefix sum
            const int16_t* cf = s_coef + min(tid, kPassBlocks - 1) * kCoefLd;
            int pred = 0, ch = 0;
            if (tid < nb) {
                const int mcu = tid / 6, k = tid - mcu * 6;
                ch = k >= 4;
                if (k >= 1 && k <= 3)
                    pred = cf[-kCoefLd];
                else if (k == 0)
                    pred = mcu ? cf[-3 * kCoefLd] : s_lastdc[0];
                else
                    pred = mcu ? cf[-6 * kCoefLd] : s_lastdc[k - 3];
            }
            Sink sink{s_bits, 0, 0, 0};
            const int len = tid < nb ? code_block<false>(cf, pred, s_dc[ch], s_ac[ch], sink) : 0;
            int total;
            const int start = wg_scan_excl(len, s_scan, tid, total);
            const int carry_n = s_carry[0];
            const int pass_bits = carry_n + total;
            // 5. the bits into the zeroed buffer (the staging of steps 1 - 3 is dead: the scan's barriers lie behind its last read)
            for (int i = tid; i < (pass_bits + 31) / 32 + 1; i += kThreads) s_bits[i] = 0;
            __syncthreads();
            if (tid < nb) {
                sink.w = (carry_n + start) >> 5, sink.n = (carry_n + start) & 31;
                code_block<true>(cf, pred, s_dc[ch], s_ac[ch], sink);
                sink.flush();
            }
            int nbytes = pass_bits >> 3;
            const int rem = pass_bits & 7;
            if (tid == 0) {
                if (carry_n) atomicOr(&s_bits[0], (uint32_t)s_carry[1] << (32 - carry_n));
                if (last && rem) atomicOr(&s_bits[pass_bits >> 5], ((1u << (8 - rem)) - 1u) << (32 - (pass_bits & 31) - (8 - rem)));   // 1-bits
            }
            if (last && rem) ++nbytes;
            __syncthreads();
            // 6. whole bytes out, 0x00 behind every 0xFF
            auto byte_at = [&](int j) { return (s_bits[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu; };
            const int cs = (nbytes + kThreads - 1) / kThreads;
            const int j0 = min(tid * cs, nbytes), j1 = min(j0 + cs, nbytes);
            int ff = 0;
            for (int j = j0; j < j1; ++j) ff += byte_at(j) == 0xFFu;
            int ff_total;
            const int ff_before = wg_scan_excl(ff, s_scan, tid, ff_total);
            if constexpr (WRITE) {
                int64_t o = out_run + j0 + ff_before;
                for (int j = j0; j < j1; ++j) {
                    const uint32_t v = byte_at(j);
                    if (o < limit) dst[o] = (uint8_t)v;
                    ++o;
                    if (v == 0xFFu) {
                        if (o < limit) dst[o] = 0;
                        ++o;
                    }
                }
            }
            out_run += nbytes + ff_total;
            if (tid == 0) {
                s_lastdc[0] = s_coef[(nb - 3) * kCoefLd], s_lastdc[1] = s_coef[(nb - 2) * kCoefLd], s_lastdc[2] = s_coef[(nb - 1) * kCoefLd];
                s_carry[0] = last ? 0 : rem;
                s_carry[1] = last || !rem ? 0 : (int)(byte_at(nbytes) >> (8 - rem));
            }
            __syncthreads();
        }
        if (row < a.rows - 1) {                                                  // RSTm between the intervals of a frame
            if (WRITE && tid == 0) {
                if (out_run < limit) dst[out_run] = 0xFF;
                if (out_run + 1 < limit) dst[out_run + 1] = (uint8_t)(0xD0 + (row & 7));
            }
            out_run += 2;
        }
        if (!WRITE && tid == 0) a.sizes[u] = (int32_t)out_run;
    }
}

int check(const void* x, int dtype, int C, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, int rescale, int quality) {
    if (!x || T < 1 || (dtype != 0 && dtype != 1) || (C != 1 && C != 3) || (rescale != 0 && rescale != 1)) return HV_ERR_ARG;
    if (quality < 1 || quality > 100 || W < 1 || H < 1 || W > HV_YUV_MAX_SIDE || H > HV_YUV_MAX_SIDE) return HV_ERR_ARG;
    if (((uintptr_t)x & (dtype == 0 ? 1 : 3)) != 0 || sc < 0 || st < 0 || sh < 0) return HV_ERR_ARG;
    return HV_OK;
}

template <bool WRITE>
int launch(Args a, int dtype, int T, hipStream_t stream) {
    a.mcus = (a.W + HV_MJPEG_MCU - 1) / HV_MJPEG_MCU, a.rows = (a.H + HV_MJPEG_MCU - 1) / HV_MJPEG_MCU;
    a.units = (int64_t)T * a.rows;
    const dim3 grid((unsigned)(a.units < kMaxWgs ? a.units : kMaxWgs));
    if (dtype == 0)
        mjpeg_kernel<uint16_t, WRITE><<<grid, dim3(kThreads), 0, stream>>>(a);
    else
        mjpeg_kernel<uint32_t, WRITE><<<grid, dim3(kThreads), 0, stream>>>(a);
    return hv_check_launch();
}

}  // namespace

extern "C" int hv_mjpeg_measure(const void* x, int dtype, int C, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, int rescale,
                                int quality, int32_t* interval_bytes, hipStream_t stream) {
    if (!interval_bytes || ((uintptr_t)interval_bytes & 3) != 0) return HV_ERR_ARG;
    if (check(x, dtype, C, sc, st, sh, T, H, W, rescale, quality) != HV_OK) return HV_ERR_ARG;
    return launch<false>(Args{x, sc, st, sh, C, rescale, H, W, quality, 0, 0, 0, interval_bytes, nullptr, nullptr}, dtype, T, stream);
}

extern "C" int hv_mjpeg_write(const void* x, int dtype, int C, int64_t sc, int64_t st, int64_t sh, int T, int H, int W, int rescale,
                              int quality, const int64_t* offsets, void* scan, hipStream_t stream) {
    if (!offsets || !scan || ((uintptr_t)offsets & 7) != 0) return HV_ERR_ARG;
    if (check(x, dtype, C, sc, st, sh, T, H, W, rescale, quality) != HV_OK) return HV_ERR_ARG;
    return launch<true>(Args{x, sc, st, sh, C, rescale, H, W, quality, 0, 0, 0, nullptr, offsets, (uint8_t*)scan}, dtype, T, stream);
}
