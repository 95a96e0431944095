// Adaptive tile selection (include/hv_attn_select.h): the CSR key-tile lists of the sliding-tile attention kernel, chosen per call from
// the pooled Q.K.  The header is the description of the rule, the outputs and the refusals; DESIGN.md section 4 has the reasons.
//
//   pool_kernel     (tile, head, q | k): thread = (row group rg = tid >> 4, 16-byte column piece cp = tid & 15); 16 rows per pass, every
//                   lane sums 8 columns in fp32; the 16 row groups are folded through LDS in the order 0 .. 15; mean = sum / count.
//   select_kernel   (band of 32 query tiles, head), 4 waves.  Phase 1: lane = (lr = lane & 31, lk = lane >> 5) holds columns
//                   [64 lk, 64 lk + 64) of qbar row i0 + lr in 64 registers; wave w takes the key blocks w, w + 4, ..: per block 64
//                   v_mfma_f32_32x32x2_f32 whose k pair is (ks, 64 + ks), so that a lane's operands are one contiguous 256-byte read of
//                   its row (the dot product's order is free: the contract bounds it by absolute sums).  Scores go to LDS, S[32][pitch].
//                   Phase 2: wave w owns rows 8 w .. 8 w + 7; lane holds the row's columns lane + 64 t, t < 16, as (e = exp2(s - max),
//                   key = the integer image of e: bits + 1, own tile 0xFFFFFFFF, no tile 0).  `tally(T)` = (mass, count) of key >= T, one
//                   butterfly each.  The cdf cut bisects T on the mass, the clamped count n bisects T on the count; elements with key > T
//                   are taken, those with key == T in ascending tile index until n is reached (ballot + popcount prefix).  e is clamped
//                   into [0, 1], so whatever the inputs hold the count tallies are exact, n bits are set, and nothing downstream can
//                   leave its slice.
//   scan_kernel     one workgroup: thread t sums a contiguous run of the n_heads * n_tiles lengths, one wg_scan_excl over the 256 run
//                   sums, then it writes its run's row pointers (and each head's closing pointer).
//   compact_kernel  a wave per (h, i): lane w < words expands bitmask word w behind the popcount prefix of the words before it.
#include "hv_common.hpp"
#include "hv_wg_scan.hpp"
#include "../../include/hv_attn_select.h"

namespace {

constexpr int D = 128;
constexpr int MAX_TILES = HV_ATTN_SELECT_MAX_TILES;
constexpr int BAND = HV_ATTN_SELECT_BAND;
constexpr int T16 = MAX_TILES / 64;               // columns of a score row a lane holds
constexpr uint32_t KEY_OWN = 0xFFFFFFFFu;         // the own tile ranks first
constexpr uint32_t KEY_TOP = 0x3F800002u;         // above the key of e = 1.0 (0x3F800000 + 1): only the own tile is >= KEY_TOP
constexpr int SEL_LDS_MAX = BAND * MAX_TILES * 4; // 131072 bytes: the score rows of a band at the largest n_tiles
static_assert(BAND == 32 && MAX_TILES % 64 == 0 && MAX_TILES <= 2048, "a band is one MFMA block; a bitmask row is at most 64 words");

__device__ __forceinline__ int words_of(int nt) { return 2 * ((nt + 63) / 64); }

// ---------------------------------------------------------------------------------------------------------------- pool
struct PoolArgs {
    const bf16_t *q, *k;
    int64_t sq, sk;
    const int *perm, *tile_start;
    float *qbar, *kbar;
    int n_tiles;
};

__global__ __launch_bounds__(256) void pool_kernel(PoolArgs a) {
    __shared__ float red[16][D + 4];
    const int i = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, rg = tid >> 4, cp = tid & 15;
    const bf16_t* src = blockIdx.z ? a.k : a.q;
    const int64_t stride = blockIdx.z ? a.sk : a.sq;
    const int s0 = a.tile_start[i], c = a.tile_start[i + 1] - s0;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = rg; s < c; s += 16) {
        const int row = a.perm[s0 + s];
        const u32x4 w = *reinterpret_cast<const u32x4*>(src + (int64_t)row * stride + h * D + cp * 8);
        float f[8];
        unpack8(w, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rg][cp * 8 + e] = acc[e];
    __syncthreads();
    if (tid < D) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += red[r][tid];
        (blockIdx.z ? a.kbar : a.qbar)[((int64_t)h * a.n_tiles + i) * D + tid] = sum / (float)c;
    }
}

// -------------------------------------------------------------------------------------------------------------- select
struct SelArgs {
    const float *qbar, *kbar;
    const int* tile_start;
    int* counts;
    uint32_t* masks;
    float* kept;
    int n_tiles, k_min, k_max;
    float sl2, cdf;
};

struct Tally {
    float mass;
    int cnt;
};
// (mass, count) of the row's elements with key >= T (T >= 1: a lane's slots without a tile have key 0)
__device__ __forceinline__ Tally tally(const uint32_t (&key)[T16], const float (&e)[T16], uint32_t T) {
    float m = 0.f;
    int c = 0;
#pragma unroll
    for (int t = 0; t < T16; ++t) {
        const bool in = key[t] >= T;
        m += in ? e[t] : 0.f;
        c += in ? 1 : 0;
    }
    return Tally{wave_sum(m), wave_sum(c)};
}

__global__ __launch_bounds__(256) void select_kernel(SelArgs a) {
    extern __shared__ float S[];
    const int nt = a.n_tiles, nkb = (nt + 31) / 32, pitch = nkb * 32, W = words_of(nt);
    const int i0 = blockIdx.x * BAND, h = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 31, lk = lane >> 5;

    // ---- phase 1: S[row][j] = sl2 * (qbar_{i0 + row} . kbar_j) + log2(c_j)
    {
        const float* qp = a.qbar + ((int64_t)h * nt + min(i0 + lr, nt - 1)) * D + lk * 64;
        f32x4 av[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) av[v] = *reinterpret_cast<const f32x4*>(qp + 4 * v);
        for (int kb = wave; kb < nkb; kb += 4) {
            const int j = kb * 32 + lr;
            const bool jv = j < nt;
            const int jc = jv ? j : nt - 1;
            const float* kp = a.kbar + ((int64_t)h * nt + jc) * D + lk * 64;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(kp + 4 * v);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v][e], bv[e], acc, 0, 0, 0);
            }
            const float lc = __log2f((float)(a.tile_start[jc + 1] - a.tile_start[jc]));
            if (jv) {
#pragma unroll
                for (int r = 0; r < 16; ++r) S[f32tile::acc_row(r, lk) * pitch + j] = __fmaf_rn(a.sl2, acc[r], lc);
            }
        }
    }
    __syncthreads();

    // ---- phase 2: a wave per row
    const uint64_t below = (1ull << lane) - 1ull;
    for (int rr = 0; rr < BAND / 4; ++rr) {
        const int row = wave * (BAND / 4) + rr, i = i0 + row;
        if (i >= nt) break;
        float e[T16];
        uint32_t key[T16];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < T16; ++t) {
            const int j = lane + 64 * t;
            e[t] = j < nt ? S[row * pitch + j] : -INFINITY;
            mx = fmaxf(mx, e[t]);
        }
        mx = wave_max(mx);
#pragma unroll
        for (int t = 0; t < T16; ++t) {
            const int j = lane + 64 * t;
            const bool valid = j < nt;
            // into [0, 1] whatever the inputs hold (fmaxf / fminf drop a NaN): the keys then lie in [1, KEY_TOP) and the count tallies are exact
            e[t] = valid ? fminf(fmaxf(__builtin_amdgcn_exp2f(e[t] - mx), 0.f), 1.f) : 0.f;
            key[t] = !valid ? 0u : j == i ? KEY_OWN : __float_as_uint(e[t]) + 1u;
        }
        const float l = tally(key, e, 1u).mass;

        // the cdf cut: the shortest prefix of the ranking whose mass reaches cdf * l
        int n = nt;
        if (a.cdf < 1.f) {
            const float target = a.cdf * l;
            uint32_t lo = 1u, hi = KEY_TOP;             // mass(key >= lo) >= target > mass(key >= hi)
            if (tally(key, e, hi).mass >= target) {
                n = 1;
            } else {
                while (hi - lo > 1u) {
                    const uint32_t mid = lo + (hi - lo) / 2u;
                    if (tally(key, e, mid).mass >= target) lo = mid; else hi = mid;
                }
                const Tally above = tally(key, e, hi), with = tally(key, e, lo);
                const int n_eq = with.cnt - above.cnt;  // the elements at the cut value enter by tile index, one at a time
                const float ev = __uint_as_float(lo - 1u);
                int ties = n_eq;
                for (int x = 1; x < n_eq; ++x)
                    if (above.mass + (float)x * ev >= target) {
                        ties = x;
                        break;
                    }
                n = above.cnt + ties;
            }
        }
        n = min(max(n, min(a.k_min, nt)), min(a.k_max, nt));
        n = min(max(n, 1), nt);

        // the first n of the ranking: every key > T, and the first `ties` of key == T by tile index
        uint32_t T = 1u;
        int ties = nt;
        if (n < nt && n == 1) {
            T = KEY_OWN, ties = 1;
        } else if (n < nt) {
            uint32_t lo = 1u, hi = KEY_TOP;             // count(key >= lo) >= n > count(key >= hi) = 1
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (tally(key, e, mid).cnt >= n) lo = mid; else hi = mid;
            }
            T = lo, ties = n - tally(key, e, hi).cnt;
        }
        const int64_t g = (int64_t)h * nt + i;
        int seen = 0;
        float km = 0.f;
#pragma unroll
        for (int t = 0; t < T16; ++t) {
            const bool eq = key[t] == T;
            const uint64_t b = __ballot(eq);
            const bool sel = key[t] > T || (eq && seen + __popcll(b & below) < ties);
            seen += __popcll(b);
            const uint64_t sb = __ballot(sel);
            km += sel ? e[t] : 0.f;
            if (lane == 0 && 2 * t < W) {
                a.masks[g * W + 2 * t] = (uint32_t)sb;
                a.masks[g * W + 2 * t + 1] = (uint32_t)(sb >> 32);
            }
        }
        km = wave_sum(km);
        if (lane == 0) {
            a.counts[g] = n;
            if (a.kept) a.kept[g] = km / l;
        }
    }
}

// -------------------------------------------------------------------------------------------------------- scan, compact
__global__ __launch_bounds__(kWgScanThreads) void scan_kernel(const int* counts, int* nb_ptr, int nt, int rows) {
    __shared__ int s[kWgScanThreads];
    const int tid = threadIdx.x, per = (rows + kWgScanThreads - 1) / kWgScanThreads;
    const int lo = min(tid * per, rows), hi = min(lo + per, rows);
    int sum = 0;
    for (int g = lo; g < hi; ++g) sum += counts[g];
    int total;
    int ex = wg_scan_excl(sum, s, tid, total);
    for (int g = lo; g < hi; ++g) {
        const int h = g / nt, i = g - h * nt;
        nb_ptr[(int64_t)h * (nt + 1) + i] = ex;
        ex += counts[g];
        if (i == nt - 1) nb_ptr[(int64_t)h * (nt + 1) + nt] = ex;
    }
}

__global__ __launch_bounds__(256) void compact_kernel(const uint32_t* masks, const int* nb_ptr, int* nb_idx, int nt, int rows, int64_t cap) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, W = words_of(nt);
    if (g >= rows) return;
    const int h = g / nt, i = g - h * nt;
    uint32_t w = lane < W ? masks[(int64_t)g * W + lane] : 0u;
    const int pc = __popc(w);
    int inc = pc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    int64_t pos = (int64_t)nb_ptr[(int64_t)h * (nt + 1) + i] + inc - pc;
    while (w) {
        const int b = __ffs(w) - 1;
        w &= w - 1u;
        if (pos >= 0 && pos < cap) nb_idx[pos] = lane * 32 + b;   // in range by construction; the test costs nothing
        ++pos;
    }
}

// workspace: qbar, kbar [H][nt][128] fp32 | counts [H * nt] int32 (padded to 16 bytes) | masks [H * nt][words] uint32
struct Layout {
    int64_t bar, counts, masks, total;
};
static Layout layout(int nt, int H) {
    const int64_t rows = (int64_t)H * nt, words = 2 * ((nt + 63) / 64);
    Layout L;
    L.bar = rows * D * 4;
    L.counts = 2 * L.bar;
    L.masks = L.counts + ((rows * 4 + 15) & ~(int64_t)15);
    L.total = L.masks + rows * words * 4;
    return L;
}
static bool shape_ok(int nt, int H) { return nt > 0 && nt <= MAX_TILES && H > 0 && H <= 65535; }

}  // namespace

extern "C" int64_t hv_attn_select_workspace_bytes(int n_tiles, int n_heads) {
    return shape_ok(n_tiles, n_heads) ? layout(n_tiles, n_heads).total : 0;
}

extern "C" int hv_attn_select_tiles(const void* q, const void* k, int64_t stride_q, int64_t stride_k, int n_q, int n_heads, int head_dim,
                                    float scale, const int* perm, const int* tile_start, int n_tiles, float cdf, int k_min, int k_max,
                                    int* nb_ptr, int* nb_idx, int64_t nb_idx_capacity, float* kept_mass, void* workspace,
                                    int64_t workspace_bytes, hipStream_t stream) {
    if (!q || !k || !perm || !tile_start || !nb_ptr || !nb_idx || !workspace || !hv_aligned16(q) || !hv_aligned16(k) ||
        !hv_aligned16(workspace) || head_dim != D || !shape_ok(n_tiles, n_heads) || n_tiles > n_q || (stride_q & 7) || (stride_k & 7) ||
        !(cdf > 0.f && cdf <= 1.f) || k_min < 1 || k_min > k_max)
        return HV_ERR_ARG;
    const int64_t rows = (int64_t)n_heads * n_tiles, most = rows * (k_max < n_tiles ? k_max : n_tiles);
    const Layout L = layout(n_tiles, n_heads);
    if (most > 0x7fffffff || nb_idx_capacity < most || workspace_bytes < L.total) return HV_ERR_ARG;
    static HvPerDeviceOnce once;
    char* ws = (char*)workspace;
    PoolArgs p;
    p.q = (const bf16_t*)q, p.k = (const bf16_t*)k, p.sq = stride_q, p.sk = stride_k, p.perm = perm, p.tile_start = tile_start;
    p.qbar = (float*)ws, p.kbar = (float*)(ws + L.bar), p.n_tiles = n_tiles;
    SelArgs s;
    s.qbar = p.qbar, s.kbar = p.kbar, s.tile_start = tile_start, s.counts = (int*)(ws + L.counts), s.masks = (uint32_t*)(ws + L.masks);
    s.kept = kept_mass, s.n_tiles = n_tiles, s.k_min = k_min, s.k_max = k_max, s.sl2 = scale * 1.4426950408889634f, s.cdf = cdf;
    if (hv_set_max_lds(once, (const void*)select_kernel, SEL_LDS_MAX) != HV_OK) return HV_ERR_LAUNCH;
    const int bands = (n_tiles + BAND - 1) / BAND;
    pool_kernel<<<dim3((unsigned)n_tiles, (unsigned)n_heads, 2), dim3(256), 0, stream>>>(p);
    select_kernel<<<dim3((unsigned)bands, (unsigned)n_heads), dim3(256), (size_t)BAND * bands * 32 * 4, stream>>>(s);
    scan_kernel<<<dim3(1), dim3(kWgScanThreads), 0, stream>>>(s.counts, nb_ptr, n_tiles, (int)rows);
    compact_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream>>>(s.masks, nb_ptr, nb_idx, n_tiles, (int)rows, nb_idx_capacity);
    return hv_check_launch();
}
