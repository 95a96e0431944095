// FP8 attention forward (include/hv_attn_fp8.h): the preparation stage (statistics, e4m3 quantisation of Q, centred K and transposed,
// permuted V into one workspace) and the attention kernel on v_mfma_scale_f32_32x32x64_f8f6f4.  The header is the description of the
// arithmetic, the workspace layout and the V-tile permutation; this file follows its names.
#include "hv_common.hpp"
#include "../../include/hv_attn_fp8.h"

namespace {

constexpr int D = 128;
constexpr int KVT = HV_ATTN_FP8_KVT;
constexpr int BM = HV_ATTN_FP8_BM;
constexpr int RING = HV_ATTN_FP8_RING;
constexpr int SBK = HV_ATTN_FP8_STAT_KEYS;
constexpr int QB = BM / 128;                  // 32-row query blocks per wave (4 waves)
constexpr int TILE_BYTES = KVT * D;           // a K tile and a V^T tile in the workspace: 8 KiB each
constexpr int MAX_KV = 0x7fffffff - 2048;
static_assert(KVT == 64 && RING == 3 && QB >= 1 && BM == QB * 128, "the kernel is written for 64-key tiles and a ring of three");

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

// ---------------------------------------------------------------------------------------------------------------- workspace
struct Layout {
    int64_t kmean, sv, sk, sq, part, q8, k8, v8, total;
    int ntile, nblk;
};
inline int64_t up(int64_t x) { return (x + HV_ATTN_FP8_ALIGN - 1) / HV_ATTN_FP8_ALIGN * HV_ATTN_FP8_ALIGN; }

bool extents_ok(int n_q, int n_kv, int n_heads) {
    return n_q >= 0 && n_heads > 0 && n_heads <= 65535 && n_kv >= 0 && n_kv <= MAX_KV && !(n_q > 0 && n_kv == 0) &&
           hv_grid_x_ok((((int64_t)n_q + BM - 1) / BM) * n_heads) && hv_grid_x_ok(((int64_t)n_q * n_heads + 15) / 16);
}

Layout layout(int n_q, int n_kv, int H) {
    Layout L;
    L.ntile = (int)(((int64_t)n_kv + KVT - 1) / KVT);
    L.nblk = (int)(((int64_t)n_kv + SBK - 1) / SBK);
    int64_t at = 0;
    L.kmean = at, at = up(at + (int64_t)H * D * 4);
    L.sv = at, at = up(at + (int64_t)H * D * 4);
    L.sk = at, at = up(at + (int64_t)H * L.ntile * 4);
    L.sq = at, at = up(at + (int64_t)n_q * H * 4);
    L.part = at, at = up(at + (int64_t)H * L.nblk * 2 * D * 4);
    L.q8 = at, at = up(at + (int64_t)n_q * H * D);
    L.k8 = at, at = up(at + (int64_t)H * L.ntile * TILE_BYTES);
    L.v8 = at, at = up(at + (int64_t)H * L.ntile * TILE_BYTES);
    L.total = at;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- e4m3
// (the pack of csrc/hv_rowwise.hip, a local copy: that file's machine code stays what it is)
__device__ __forceinline__ uint32_t pack4_e4m3(float a, float b, float c, float d) {
    uint32_t w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return w;
}
constexpr float MIN_SCALE = 1.17549435e-38f;   // 2^-126
__device__ __forceinline__ float scale_of(float amax) { return amax > 0.f ? fmaxf(amax * (1.0f / 448.0f), MIN_SCALE) : 1.0f; }
__device__ __forceinline__ float clamp448(float v) { return __builtin_amdgcn_fmed3f(v, -448.0f, 448.0f); }

// ---------------------------------------------------------------------------------------------------------------- statistics
// level 1: one workgroup per (block of SBK keys, head); wave c runs chain c, a lane owns two adjacent channels
__global__ __launch_bounds__(256) void stat_partial_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t sk,
                                                            int64_t sv, int n_kv, int nblk, float* __restrict__ part) {
    __shared__ float sh[4][2][D];
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6, h = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * SBK;
    const int64_t k1 = k0 + SBK < n_kv ? k0 + SBK : n_kv;
    float s0 = 0.f, s1 = 0.f, m0 = 0.f, m1 = 0.f;
    for (int64_t j = k0 + c; j < k1; j += 4) {
        const uint32_t kw = *reinterpret_cast<const uint32_t*>(k + j * sk + h * D + lane * 2);
        const uint32_t vw = *reinterpret_cast<const uint32_t*>(v + j * sv + h * D + lane * 2);
        s0 += bf2f_lo(kw), s1 += bf2f_hi(kw);
        m0 = fmaxf(m0, fabsf(bf2f_lo(vw))), m1 = fmaxf(m1, fabsf(bf2f_hi(vw)));
    }
    sh[c][0][lane * 2] = s0, sh[c][0][lane * 2 + 1] = s1;
    sh[c][1][lane * 2] = m0, sh[c][1][lane * 2 + 1] = m1;
    __syncthreads();
    if (threadIdx.x < D) {
        const int d = threadIdx.x;
        float* out = part + ((int64_t)h * nblk + blockIdx.x) * 2 * D;
        out[d] = (sh[0][0][d] + sh[1][0][d]) + (sh[2][0][d] + sh[3][0][d]);
        out[D + d] = fmaxf(fmaxf(sh[0][1][d], sh[1][1][d]), fmaxf(sh[2][1][d], sh[3][1][d]));
    }
}

// level 2: one workgroup per head, a thread per channel, the blocks in ascending order
__global__ __launch_bounds__(D) void stat_final_kernel(const float* __restrict__ part, int n_kv, int nblk, float* __restrict__ kmean,
                                                        float* __restrict__ sv) {
    const int d = threadIdx.x, h = blockIdx.x;
    float s = 0.f, m = 0.f;
    for (int b = 0; b < nblk; ++b) {
        const float* p = part + ((int64_t)h * nblk + b) * 2 * D;
        s += p[d];
        m = fmaxf(m, p[D + d]);
    }
    kmean[h * D + d] = __fdiv_rn(s, (float)n_kv);
    sv[h * D + d] = scale_of(m);
}

// ---------------------------------------------------------------------------------------------------------------- Q
// 16 lanes per (token, head) row of 128, 8 channels a lane
__global__ __launch_bounds__(256) void quant_q_kernel(const bf16_t* __restrict__ q, int64_t stride_q, int64_t n_rows, int H, float c,
                                                       uint8_t* __restrict__ q8, float* __restrict__ sq) {
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int sub = threadIdx.x & 15;
    if (row >= n_rows) return;
    const int64_t tok = row / H;
    const int h = (int)(row - tok * H);
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(q + tok * stride_q + h * D + sub * 8), f);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        f[j] = __fmul_rn(f[j], c);
        amax = fmaxf(amax, fabsf(f[j]));
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float s = scale_of(amax);
    const float inv = __fdiv_rn(1.0f, s);
    if (sub == 0) sq[row] = s;
    u32x2 w;
    w[0] = pack4_e4m3(clamp448(f[0] * inv), clamp448(f[1] * inv), clamp448(f[2] * inv), clamp448(f[3] * inv));
    w[1] = pack4_e4m3(clamp448(f[4] * inv), clamp448(f[5] * inv), clamp448(f[6] * inv), clamp448(f[7] * inv));
    *reinterpret_cast<u32x2*>(q8 + row * D + sub * 8) = w;
}

// ---------------------------------------------------------------------------------------------------------------- K and V
// key position p of a V^T tile row -> key of the tile (the header's permutation)
__device__ __forceinline__ int v_key_of(int p) { return 32 * ((p >> 4) & 1) + 8 * ((p >> 2) & 3) + 4 * (p >> 5) + (p & 3); }

// one workgroup per (key tile, head): thread = (key row tid >> 2, 32-channel quarter tid & 3)
__global__ __launch_bounds__(256) void quant_kv_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t stride_k,
                                                        int64_t stride_v, int n_kv, int ntile, const float* __restrict__ kmean,
                                                        const float* __restrict__ svp, float* __restrict__ skp,
                                                        uint8_t* __restrict__ k8, uint8_t* __restrict__ v8) {
    constexpr int VP = D + 16;                                        // pitch of the staged V codes (16-byte rows)
    __shared__ __attribute__((aligned(16))) uint8_t vs[KVT * VP];
    __shared__ float wmax[4];
    const int tid = threadIdx.x, r = tid >> 2, qd = tid & 3, h = blockIdx.y, t = blockIdx.x;
    const int64_t key = (int64_t)t * KVT + r;
    const bool valid = key < n_kv;
    float kc[32], vf[32];
    float amax = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int d0 = qd * 32 + c * 8;
        float a[8] = {}, b[8] = {};
        if (valid) {
            unpack8(*reinterpret_cast<const u32x4*>(k + key * stride_k + h * D + d0), a);
            unpack8(*reinterpret_cast<const u32x4*>(v + key * stride_v + h * D + d0), b);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            kc[c * 8 + j] = valid ? __fsub_rn(a[j], kmean[h * D + d0 + j]) : 0.f;
            vf[c * 8 + j] = valid ? b[j] * __fdiv_rn(1.0f, svp[h * D + d0 + j]) : 0.f;
            amax = fmaxf(amax, fabsf(kc[c * 8 + j]));
        }
    }
    amax = wave_max(amax);
    if ((tid & 63) == 0) wmax[tid >> 6] = amax;
    __syncthreads();
    const float s = scale_of(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])));
    const float inv = __fdiv_rn(1.0f, s);
    if (tid == 0) skp[(int64_t)h * ntile + t] = s;
    uint8_t* kout = k8 + ((int64_t)h * ntile + t) * TILE_BYTES + r * D + qd * 32;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        u32x4 wk, wv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = c * 16 + i * 4;
            wk[i] = pack4_e4m3(clamp448(kc[e] * inv), clamp448(kc[e + 1] * inv), clamp448(kc[e + 2] * inv), clamp448(kc[e + 3] * inv));
            wv[i] = pack4_e4m3(clamp448(vf[e]), clamp448(vf[e + 1]), clamp448(vf[e + 2]), clamp448(vf[e + 3]));
        }
        *reinterpret_cast<u32x4*>(kout + c * 16) = wk;
        *reinterpret_cast<u32x4*>(vs + r * VP + qd * 32 + c * 16) = wv;
    }
    __syncthreads();
    // transposed, permuted store: thread = (channel tid >> 1, half g = tid & 1) writes positions 32 g .. 32 g + 31 of row d
    const int d = tid >> 1, g = tid & 1;
    uint8_t* vout = v8 + ((int64_t)h * ntile + t) * TILE_BYTES + d * KVT + g * 32;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        u32x4 w;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t x = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) x |= (uint32_t)vs[v_key_of(g * 32 + c * 16 + i * 4 + e) * VP + d] << (8 * e);
            w[i] = x;
        }
        *reinterpret_cast<u32x4*>(vout + c * 16) = w;
    }
}

// ---------------------------------------------------------------------------------------------------------------- attention
__device__ __forceinline__ i32x8 load32(const uint8_t* p) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(p), hi = *reinterpret_cast<const i32x4*>(p + 16);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ f32x16 mfma8(i32x8 a, i32x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0 /*A: e4m3*/, 0 /*B: e4m3*/, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}

constexpr int KP = D + 16, VP = KVT + 16;                 // LDS row pitches of a K tile (64 rows) and a V^T tile (128 rows)
constexpr int KB = KVT * KP, STAGE = KB + D * VP;         // 9216 + 10240 bytes a stage
static_assert(RING * STAGE <= 65536, "the ring must fit the static LDS limit");

struct Fp8Args {
    const uint8_t *q8, *k8, *v8;
    const float *sq, *sk, *sv;
    bf16_t* o;
    int64_t so;
    int n_q, n_kv, H, ntile, n_qtiles;
};

__global__ __launch_bounds__(256) void attn_fp8_kernel(Fp8Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[RING * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, g = lane >> 5;
    const int h = blockIdx.x / a.n_qtiles, qt = blockIdx.x - h * a.n_qtiles;     // the q-tiles of a head are neighbours: K/V stay in L2
    const int64_t q0 = (int64_t)qt * BM + wave * (32 * QB);

    // Q fragments (B operands) and row scales: a lane is query column j of each of its blocks; rows behind n_q are zeros
    i32x8 bq[QB][2];
    float sqv[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int64_t row = q0 + qb * 32 + j;
        const bool ok = row < a.n_q;
        const int64_t at = ok ? row * a.H + h : 0;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            const i32x8 w = load32(a.q8 + at * D + dh * 64 + g * 32);
            bq[qb][dh] = ok ? w : i32x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
        sqv[qb] = ok ? a.sq[at] : 0.f;
    }

    const uint8_t* kt = a.k8 + (int64_t)h * a.ntile * TILE_BYTES;
    const uint8_t* vt = a.v8 + (int64_t)h * a.ntile * TILE_BYTES;
    const float* skh = a.sk + (int64_t)h * a.ntile;
    // a thread moves 2 x 16 bytes of the K tile and of the V^T tile: chunks tid and tid + 256
    u32x4 st[4];
    auto fetch = [&](int t) {
        const uint8_t *kp = kt + (int64_t)t * TILE_BYTES, *vp = vt + (int64_t)t * TILE_BYTES;
        st[0] = *reinterpret_cast<const u32x4*>(kp + tid * 16);
        st[1] = *reinterpret_cast<const u32x4*>(kp + (tid + 256) * 16);
        st[2] = *reinterpret_cast<const u32x4*>(vp + tid * 16);
        st[3] = *reinterpret_cast<const u32x4*>(vp + (tid + 256) * 16);
    };
    auto stash = [&](int stage) {
        uint8_t* s = lds + stage * STAGE;
        const int c0 = tid, c1 = tid + 256;
        *reinterpret_cast<u32x4*>(s + (c0 >> 3) * KP + (c0 & 7) * 16) = st[0];
        *reinterpret_cast<u32x4*>(s + (c1 >> 3) * KP + (c1 & 7) * 16) = st[1];
        *reinterpret_cast<u32x4*>(s + KB + (c0 >> 2) * VP + (c0 & 3) * 16) = st[2];
        *reinterpret_cast<u32x4*>(s + KB + (c1 >> 2) * VP + (c1 & 3) * 16) = st[3];
    };
    fetch(0), stash(0);
    if (a.ntile > 1) fetch(1), stash(1);
    __syncthreads();

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 oacc[QB][4];
    float m[QB], l[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m[qb] = -INFINITY, l[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < 4; ++db) oacc[qb][db] = zero;
    }

    int stage = 0;
    for (int t = 0; t < a.ntile; ++t) {
        const bool ahead = t + 2 < a.ntile;                 // uniform
        if (ahead) fetch(t + 2);
        const uint8_t* s = lds + stage * STAGE;
        const float skt = skh[t];
        // S^T = K Q^T: lane (j, g) reads bytes 32 g .. of channel half dh of key row 32 kb + j
        f32x16 sc[QB][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int dh = 0; dh < 2; ++dh) {
                const i32x8 ka = load32(s + (kb * 32 + j) * KP + dh * 64 + g * 32);
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) sc[qb][kb] = mfma8(ka, bq[qb][dh], dh == 0 ? zero : sc[qb][kb]);
            }
        const int left = a.n_kv - t * KVT;                  // valid keys from this tile on (>= 1)
        i32x8 pb[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const float f = sqv[qb] * skt;
            float mx = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float x = sc[qb][kb][r] * f;
                    if (kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g >= left) x = -INFINITY;
                    sc[qb][kb][r] = x;
                    mx = fmaxf(mx, x);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m[qb], mx);
            const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
            m[qb] = mn;
            float ls = 0.f;
            i32x8 w;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    float p[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        p[e] = __builtin_amdgcn_exp2f(sc[qb][kb][r4 * 4 + e] - mn);
                        ls += p[e];
                    }
                    w[kb * 4 + r4] = (int)pack4_e4m3(p[0] * 256.f, p[1] * 256.f, p[2] * 256.f, p[3] * 256.f);
                }
            pb[qb] = w;
            l[qb] = l[qb] * alpha + ls;
#pragma unroll
            for (int db = 0; db < 4; ++db) oacc[qb][db] *= alpha;
        }
        // O^T += V^T P^T: lane (j, g) reads key positions 32 g .. of channel row 32 db + j
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const i32x8 va = load32(s + KB + (db * 32 + j) * VP + g * 32);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) oacc[qb][db] = mfma8(va, pb[qb], oacc[qb][db]);
        }
        if (ahead) stash(stage == 0 ? 2 : stage - 1);       // the stage tile t - 1 left: (t + 2) % 3
        __syncthreads();
        stage = stage == 2 ? 0 : stage + 1;
    }

    // epilogue: the two halves of a column share its row; O[d] * sv[d] / (l * 2^8)
    const float* svh = a.sv + h * D;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const float lt = l[qb] + __shfl_xor(l[qb], 32, 64);
        const float inv = 1.0f / (lt * 256.f);
        const int64_t row = q0 + qb * 32 + j;
        if (row < a.n_q) {
            bf16_t* orow = a.o + row * a.so + h * D;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const int d = db * 32 + r4 * 8 + g * 4;
                    const f32x4 sv4 = *reinterpret_cast<const f32x4*>(svh + d);
                    u32x2 w;
                    w[0] = pack_bf2(oacc[qb][db][r4 * 4] * sv4[0] * inv, oacc[qb][db][r4 * 4 + 1] * sv4[1] * inv);
                    w[1] = pack_bf2(oacc[qb][db][r4 * 4 + 2] * sv4[2] * inv, oacc[qb][db][r4 * 4 + 3] * sv4[3] * inv);
                    *reinterpret_cast<u32x2*>(orow + d) = w;
                }
        }
    }
}

}  // namespace

extern "C" int64_t hv_attn_fp8_workspace_bytes(int n_q, int n_kv, int n_heads) {
    return extents_ok(n_q, n_kv, n_heads) ? layout(n_q, n_kv, n_heads).total : 0;
}

extern "C" int hv_attn_fp8_quantise(const void* q, const void* k, const void* v, int64_t stride_q, int64_t stride_k, int64_t stride_v,
                                    int n_q, int n_kv, int n_heads, int head_dim, float scale, void* workspace, int64_t workspace_bytes,
                                    hipStream_t stream) {
    if (!q || !k || !v || !workspace || head_dim != D || !extents_ok(n_q, n_kv, n_heads) || (stride_q & 7) || (stride_k & 7) ||
        (stride_v & 7) || !hv_aligned16(workspace))
        return HV_ERR_ARG;
    const Layout L = layout(n_q, n_kv, n_heads);
    if (workspace_bytes < L.total) return HV_ERR_ARG;
    if (n_q == 0) return HV_OK;
    char* ws = (char*)workspace;
    const bf16_t *kp = (const bf16_t*)k, *vp = (const bf16_t*)v;
    float *kmean = (float*)(ws + L.kmean), *sv = (float*)(ws + L.sv), *part = (float*)(ws + L.part);
    stat_partial_kernel<<<dim3((unsigned)L.nblk, (unsigned)n_heads), dim3(256), 0, stream>>>(kp, vp, stride_k, stride_v, n_kv, L.nblk, part);
    stat_final_kernel<<<dim3((unsigned)n_heads), dim3(D), 0, stream>>>(part, n_kv, L.nblk, kmean, sv);
    const int64_t n_rows = (int64_t)n_q * n_heads;
    quant_q_kernel<<<dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, stream>>>((const bf16_t*)q, stride_q, n_rows, n_heads,
                                                                                 scale * 1.4426950408889634f, (uint8_t*)(ws + L.q8),
                                                                                 (float*)(ws + L.sq));
    quant_kv_kernel<<<dim3((unsigned)L.ntile, (unsigned)n_heads), dim3(256), 0, stream>>>(kp, vp, stride_k, stride_v, n_kv, L.ntile, kmean, sv,
                                                                                         (float*)(ws + L.sk), (uint8_t*)(ws + L.k8),
                                                                                         (uint8_t*)(ws + L.v8));
    return hv_check_launch();
}

extern "C" int hv_attn_fwd_fp8(const void* workspace, int64_t workspace_bytes, void* o, int64_t stride_o, int n_q, int n_kv, int n_heads,
                               int head_dim, hipStream_t stream) {
    if (!workspace || !o || head_dim != D || !extents_ok(n_q, n_kv, n_heads) || (stride_o & 3) || !hv_aligned16(workspace) ||
        !hv_pitch_ok(n_q, stride_o, (int64_t)n_heads * D))
        return HV_ERR_ARG;
    const Layout L = layout(n_q, n_kv, n_heads);
    if (workspace_bytes < L.total) return HV_ERR_ARG;
    if (n_q == 0) return HV_OK;
    const char* ws = (const char*)workspace;
    Fp8Args a;
    a.q8 = (const uint8_t*)(ws + L.q8), a.k8 = (const uint8_t*)(ws + L.k8), a.v8 = (const uint8_t*)(ws + L.v8);
    a.sq = (const float*)(ws + L.sq), a.sk = (const float*)(ws + L.sk), a.sv = (const float*)(ws + L.sv);
    a.o = (bf16_t*)o, a.so = stride_o;
    a.n_q = n_q, a.n_kv = n_kv, a.H = n_heads, a.ntile = L.ntile;
    a.n_qtiles = (int)(((int64_t)n_q + BM - 1) / BM);
    attn_fp8_kernel<<<dim3((unsigned)(a.n_qtiles * n_heads)), dim3(256), 0, stream>>>(a);
    return hv_check_launch();
}
