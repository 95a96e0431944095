// Content statistics of a clip on the device: histograms of the 8-bit gray frames and of the differences of consecutive gray frames, and
// the entropy of histogram rows.  The fork's bucket lists (metric_buckets/InterEntropy_buckets/) name the measure and its edges but
// not the program that computed it; the definition here is this project's own: inter-frame entropy = Shannon entropy, in bits, of the
// histogram of gray[t+1] - gray[t], averaged over the pairs of a clip.  The gray frames are those of hv_spectrum.hip mode 0: quantise()
// (hv_common.hpp) on R, G, B, then the integer luma (wr R + wg G + wb B + round) >> shift.  They never reach HBM.
//
//   content_hist_kernel<T, VEC>  a workgroup owns one chunk of HV_CONTENT_CHUNK pixels (row-major pixel index over H x W) and walks up to
//                                8 consecutive frames of it; the previous frame's gray bytes stay in registers (4 to a dword), so a frame is
//                                read 1 + 1/F times (F = 8 once the launch is deep enough, 1 for small clips where workgroups are scarce).
//                                A thread takes quads of 4 consecutive pixels: quad j * 256 + tid of the chunk in pass j (VEC: one vector
//                                load per channel when W, the strides and the pointer allow; else element loads that follow the row
//                                break).  So: 4 pixels per thread, 256 per wave, 1024 per pass, 8 passes per chunk.
//                                Counting: every wave owns a private LDS histogram pair (256 + 511 bins), and before a wave adds a value
//                                it collapses equal ones: the first live lane's (gray, previous gray) is broadcast, the lanes that hold
//                                the same pair are counted by a ballot, and one lane adds the count to both histograms; repeated while a
//                                round retires at least 8 lanes, the rest add 1 each.  Real video puts most differences on 0 and +-1 -
//                                64 lanes on one LDS address, which the atomic unit serialises; collapsed, a constant clip costs one
//                                add per wave and histogram, random data one extra ballot (measured: tools/bench_content.py, constant
//                                1.12 x and slowly drifting 1.57 x the time of random data).  LDS atomics are vector ds_add_u32.
//   content_fold                 the four wave histograms of a (chunk, frame) are summed and stored as a partial row in the workspace
//                                [chunk][T * 256 + (T - 1) * 511]; this kernel adds the chunks of each bin in chunk order.  Every partial
//                                cell is written by exactly one workgroup, so nothing needs clearing and no global atomic is used;
//                                integers, so the bits are the same on every run and row t does not depend on T or on other frames.
//   entropy_kernel               one wave per histogram row: N, sum c v, sum c v^2 as exact 64-bit integers, sum c log2 c in fp64 (lane l
//                                takes bins l, l + 64, ... in order, then the butterfly), H = log2 N - (sum c log2 c) / N.
#include "hv_common.hpp"
#include "../../include/hv_content.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kQuad = 4;                                   // consecutive pixels of one thread
constexpr int kChunk = HV_CONTENT_CHUNK;                   // pixels of one workgroup
constexpr int kPass = kThreads * kQuad;                    // pixels of one pass of the workgroup
constexpr int kSlots = kChunk / kPass;
static_assert(kSlots * kPass == kChunk, "a chunk is whole passes");
constexpr int kIntra = 256, kInter = HV_CONTENT_INTER_BINS;
static_assert(kInter == 2 * 255 + 1, "one bin per difference of two bytes");
constexpr int kMaxWalk = 8;                                // frames a workgroup walks at most
constexpr int kWalkDepth = 1024;                           // (chunk, frame) units per walked frame before a longer walk pays
constexpr int kPeelMin = 8;                                // a collapse round must retire this many lanes to be worth the next
constexpr int kMaxT = 65535;                               // frame groups are grid.y
constexpr int kMaxEntropyBins = 1024;

struct Luma {
    int wr, wg, wb, round, shift;
};

// intra[g] += 1 and, with `pair`, inter[g - pg + 255] += 1 for every lane with `active`; called by all lanes of the wave together.  Lanes
// are collapsed on the key (g, pg): equal keys have equal bins in both histograms, so one round serves both.
__device__ __forceinline__ void hist_add(uint32_t* intra, uint32_t* inter, int g, int pg, bool pair, bool active, int lane) {
    const int key = g | (pg << 8);
    uint64_t rem = __ballot(active);
    while (rem) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)rem) - 1);
        const int k0 = __builtin_amdgcn_readlane(key, leader);
        const uint64_t same = __ballot(active && key == k0);
        const int n = __popcll(same);
        if (n < kPeelMin) break;
        if (lane == leader) {
            atomicAdd(&intra[k0 & 255], (uint32_t)n);
            if (pair) atomicAdd(&inter[(k0 & 255) - (k0 >> 8) + 255], (uint32_t)n);
        }
        active = active && key != k0;
        rem &= ~same;
    }
    if (active) {
        atomicAdd(&intra[g], 1u);
        if (pair) atomicAdd(&inter[g - pg + 255], 1u);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void content_hist_kernel(const T* __restrict__ x, int64_t sc, int64_t st, int64_t sh, int Tn,
                                                               uint32_t HW, uint32_t W, int rescale, Luma lu, int walk,
                                                               uint32_t* __restrict__ part, int64_t R) {
    __shared__ uint32_t s_intra[kWaves][kIntra];
    __shared__ uint32_t s_inter[kWaves][kInter + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t base = blockIdx.x * (uint32_t)kChunk;   // < HW <= 2^31 - 1: base + kChunk fits 32 bits
    const int t0 = blockIdx.y * walk, t1 = min(t0 + walk, Tn);
    uint32_t* my_intra = s_intra[wave];
    uint32_t* my_inter = s_inter[wave];
    uint32_t* dst = part + (int64_t)blockIdx.x * R;

    auto gray = [&](float r, float g, float b) -> uint32_t {
        return (uint32_t)((lu.wr * (int)quantise(r, rescale) + lu.wg * (int)quantise(g, rescale) + lu.wb * (int)quantise(b, rescale) +
                           lu.round) >> lu.shift);
    };

    uint32_t prev[kSlots] = {};                            // gray bytes of the frame before, pixel i of the quad in byte i
    for (int t = t0 > 0 ? t0 - 1 : 0; t < t1; ++t) {
        const bool count = t >= t0;                        // frame t0 - 1 is read for its gray alone: its rows belong to the group before
        const bool pair = count && t > 0;
        if (count) {
            for (int i = tid; i < kWaves * kIntra; i += kThreads) (&s_intra[0][0])[i] = 0;
            for (int i = tid; i < kWaves * (kInter + 1); i += kThreads) (&s_inter[0][0])[i] = 0;
            __syncthreads();
        }
        const T* xt = x + (int64_t)t * st;
        uint32_t cur[kSlots];
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            const uint32_t p0 = base + (uint32_t)(j * kThreads + tid) * kQuad;
            uint32_t g4 = 0;
            if (p0 < HW) {
                uint32_t h = p0 / W, w = p0 - h * W;
                if constexpr (VEC) {                       // W % 4 == 0: the quad lies in one row and is whole
                    typedef T vec4 __attribute__((ext_vector_type(4)));
                    const T* p = xt + (int64_t)h * sh + w;
                    const vec4 r = *(const vec4*)p, g = *(const vec4*)(p + sc), b = *(const vec4*)(p + 2 * sc);
#pragma unroll
                    for (int i = 0; i < kQuad; ++i) g4 |= gray((float)r[i], (float)g[i], (float)b[i]) << (8 * i);
                } else {
#pragma unroll
                    for (int i = 0; i < kQuad; ++i) {
                        if (p0 + i < HW) {
                            const T* p = xt + (int64_t)h * sh + w;
                            g4 |= gray((float)p[0], (float)p[sc], (float)p[2 * sc]) << (8 * i);
                            if (++w == W) {
                                w = 0;
                                ++h;
                            }
                        }
                    }
                }
            }
            cur[j] = g4;
        }
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            const uint32_t p0 = base + (uint32_t)(j * kThreads + tid) * kQuad;
            if (count && base + (uint32_t)j * kPass < HW) {          // uniform over the workgroup
#pragma unroll
                for (int i = 0; i < kQuad; ++i) {
                    const bool live = p0 + i < HW;
                    const int g = (int)((cur[j] >> (8 * i)) & 255u);
                    hist_add(my_intra, my_inter, g, pair ? (int)((prev[j] >> (8 * i)) & 255u) : 0, pair, live, lane);
                }
            }
            prev[j] = cur[j];
        }
        if (count) {
            __syncthreads();
            for (int i = tid; i < kIntra; i += kThreads) {
                uint32_t s = s_intra[0][i];
                for (int wv = 1; wv < kWaves; ++wv) s += s_intra[wv][i];
                dst[(int64_t)t * kIntra + i] = s;
            }
            if (pair) {
                for (int i = tid; i < kInter; i += kThreads) {
                    uint32_t s = s_inter[0][i];
                    for (int wv = 1; wv < kWaves; ++wv) s += s_inter[wv][i];
                    dst[(int64_t)Tn * kIntra + (int64_t)(t - 1) * kInter + i] = s;
                }
            }
            __syncthreads();
        }
    }
}

// one thread per cell of [T * 256 + (T - 1) * 511]: the chunks in order
__global__ __launch_bounds__(kThreads) void content_fold(const uint32_t* __restrict__ part, int nchunks, int64_t R, int64_t n_intra,
                                                        uint32_t* __restrict__ intra, uint32_t* __restrict__ inter) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= R) return;
    uint32_t s = 0;
    for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * R + idx];
    if (idx < n_intra) intra[idx] = s;
    else inter[idx - n_intra] = s;
}

__global__ __launch_bounds__(64) void entropy_kernel(const uint32_t* __restrict__ counts, int bins, int origin, double* __restrict__ out) {
    const int l = threadIdx.x;
    const uint32_t* c = counts + (int64_t)blockIdx.x * bins;
    unsigned long long n = 0;
    long long s1 = 0, s2 = 0;
    double e = 0.0;
    for (int b = l; b < bins; b += 64) {
        const long long k = (long long)c[b], v = b - origin;
        n += (unsigned long long)k;
        s1 += k * v;
        s2 += k * v * v;
        if (k > 1) e += (double)k * log2((double)k);       // 0 log 0 = 0, 1 log 1 = 0
    }
    n = wave_sum(n);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    e = wave_sum(e);
    if (l == 0) {
        double* o = out + (int64_t)blockIdx.x * 3;
        o[0] = n ? fmax(log2((double)n) - e / (double)n, 0.0) : 0.0;
        o[1] = (double)s1;
        o[2] = (double)s2;
    }
}

struct Plan {
    int nchunks, walk, groups;
    int64_t R, ws_bytes;
};
inline bool plan(int T, int H, int W, Plan& p) {
    if (T < 1 || T > kMaxT || H < 1 || W < 1 || H > (1 << 16) || W > (1 << 16) || (int64_t)H * W > 0x7fffffff) return false;
    const int64_t HW = (int64_t)H * W;
    p.nchunks = (int)((HW + kChunk - 1) / kChunk);
    const int64_t deep = (int64_t)p.nchunks * T / kWalkDepth;
    p.walk = (int)(deep < 1 ? 1 : deep > kMaxWalk ? kMaxWalk : deep);
    p.groups = (T + p.walk - 1) / p.walk;
    p.R = (int64_t)T * kIntra + (int64_t)(T - 1) * kInter;
    p.ws_bytes = (int64_t)p.nchunks * p.R * 4;
    return true;
}

template <typename T>
int launch(const void* x, int64_t sc, int64_t st, int64_t sh, int Tn, int H, int W, int rescale, Luma lu, uint32_t* intra, uint32_t* inter,
           uint32_t* ws, const Plan& p, hipStream_t stream) {
    const bool vec = W % kQuad == 0 && sc % kQuad == 0 && st % kQuad == 0 && sh % kQuad == 0 && ((uintptr_t)x % (kQuad * sizeof(T))) == 0;
    const dim3 grid((unsigned)p.nchunks, (unsigned)p.groups);
    const uint32_t HW = (uint32_t)((int64_t)H * W);
    if (vec)
        content_hist_kernel<T, true><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, Tn, HW, (uint32_t)W, rescale, lu, p.walk, ws, p.R);
    else
        content_hist_kernel<T, false><<<grid, dim3(kThreads), 0, stream>>>((const T*)x, sc, st, sh, Tn, HW, (uint32_t)W, rescale, lu, p.walk, ws, p.R);
    content_fold<<<dim3((unsigned)((p.R + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream>>>(ws, p.nchunks, p.R, (int64_t)Tn * kIntra, intra,
                                                                                                   inter);
    return hv_check_launch();
}

}  // namespace

extern "C" int64_t hv_content_histograms_workspace_bytes(int T, int H, int W) {
    Plan p;
    return plan(T, H, W, p) ? p.ws_bytes : 0;
}

extern "C" int hv_content_histograms(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int T, int H, int W, int rescale, int wr,
                                     int wg, int wb, int round, int shift, void* intra, void* inter, void* workspace, int64_t workspace_bytes,
                                     hipStream_t stream) {
    Plan p;
    if (!x || !intra || !workspace || (dtype != 0 && dtype != 1) || (rescale != 0 && rescale != 1) || !plan(T, H, W, p)) return HV_ERR_ARG;
    if (T > 1 && !inter) return HV_ERR_ARG;
    // rows are W contiguous elements; rows, frames and channels may be strided (views), never overlapping backwards
    if (sh < W || sc < 0 || st < 0) return HV_ERR_ARG;
    // the luma stays a byte and its int32 arithmetic cannot overflow
    if (wr < 0 || wg < 0 || wb < 0 || round < 0 || shift < 0 || shift > 22 || wr > (1 << 22) || wg > (1 << 22) || wb > (1 << 22) ||
        ((int64_t)wr + wg + wb) * 255 + round >= ((int64_t)256 << shift))
        return HV_ERR_ARG;
    if (((uintptr_t)workspace & 3) != 0 || ((uintptr_t)intra & 3) != 0 || ((uintptr_t)inter & 3) != 0 || workspace_bytes < p.ws_bytes)
        return HV_ERR_ARG;
    const Luma lu{wr, wg, wb, round, shift};
    if (dtype == 0)
        return launch<_Float16>(x, sc, st, sh, T, H, W, rescale, lu, (uint32_t*)intra, (uint32_t*)inter, (uint32_t*)workspace, p, stream);
    return launch<float>(x, sc, st, sh, T, H, W, rescale, lu, (uint32_t*)intra, (uint32_t*)inter, (uint32_t*)workspace, p, stream);
}

extern "C" int hv_histogram_entropy(const void* counts, int64_t rows, int bins, int origin, double* out, hipStream_t stream) {
    if (rows < 0 || rows > 0x7fffffff || bins < 1 || bins > kMaxEntropyBins || origin < 0 || origin > bins) return HV_ERR_ARG;
    if (rows == 0) return HV_OK;
    if (!counts || !out || ((uintptr_t)counts & 3) != 0 || ((uintptr_t)out & 7) != 0) return HV_ERR_ARG;
    entropy_kernel<<<dim3((unsigned)rows), dim3(64), 0, stream>>>((const uint32_t*)counts, bins, origin, out);
    return hv_check_launch();
}
