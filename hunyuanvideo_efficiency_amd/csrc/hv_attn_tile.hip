// Sliding-tile attention forward (include/hv_attn_tile.h): bf16 attention of one query tile against the key rows of its neighbour tiles
// (gathered through the plan's permutation) and one dense key range, on v_mfma_f32_32x32x16_bf16.  The header is the description of the
// plan, the refusals and the arithmetic contract; DESIGN.md section 4 has the LDS layout.  Plain HIP with the MFMA builtin: nothing of
// hv_attention_w4.hip is used here.
//
//   workgroup = (tile, head), 4 waves; wave = 64 query slots = two 32-row blocks qb; lane = (j = lane & 31, g = lane >> 5).
//   Per 64-key chunk and wave:  S^T[qb][kb] = K[kb] . Q'[qb]^T   2 x 2 chains of 8 MFMAs (A = K rows from LDS, B = Q' from registers)
//                               O^T[qb][db] += V^T[db] . P^T[qb] 2 x 4 tiles x 4 k-steps (A = V^T rows from LDS, B = P from registers)
//   A lane of the S^T accumulator holds query column j and keys kb*32 + (r & 3) + 8 (r >> 2) + 4 g, r = 0 .. 15.  Registers 8 hs .. 8 hs + 7
//   are the B operand of k-step a = 2 kb + hs of P.V as they stand, so P never passes through LDS; the V^T tile is stored with its key
//   positions in that order instead: key 16 a + 8 u + 4 g + w sits at position 16 a + 8 g + 4 u + w of its channel row.
//   Global -> LDS: thread (qd = lane & 15, c8 = 4 wave + (lane >> 4)) moves 8 channels c8 * 8 .. of the 4 keys 4 qd .. 4 qd + 3: four
//   16-byte reads of K, four of V; K goes to LDS as it is, V as eight 8-byte writes (4 keys of one channel each) - the transposition
//   happens in registers on the way in.
#include "hv_common.hpp"
#include "../../include/hv_attn_tile.h"

namespace {

constexpr int D = 128;
constexpr int KVT = HV_ATTN_TILE_KVT;
constexpr int BM = HV_ATTN_TILE_BM;
constexpr int RING = HV_ATTN_TILE_RING;
constexpr int MAX_KV = 0x7fffffff - 2048;
constexpr int KP = D * 2 + 16;                    // bytes of a K row in LDS (64 rows of 128 bf16): 17 x 16 bytes
constexpr int VP = KVT * 2 + 16;                  // bytes of a V^T row in LDS (128 rows of 64 bf16): 9 x 16 bytes
constexpr int KB = KVT * KP, STAGE = KB + D * VP; // 17408 + 18432 bytes a stage
constexpr int LDS_BYTES = RING * STAGE;           // 107520: dynamic LDS, one workgroup per CU
static_assert(KVT == 64 && RING == 3 && BM == 256, "the kernel is written for 64-key chunks, a ring of three and 4 waves x 64 rows");

struct TileArgs {
    const bf16_t *q, *k, *v;
    bf16_t* o;
    int64_t sq, sk, sv, so;
    const int *perm, *tile_start, *nb_ptr, *nb_idx;
    int n_tiles, per_head, dense_lo, dense_hi;
    float scale_log2e;
};

struct Chunk {
    int base, valid;      // first slot (gathered) or first row (dense) and the number of valid keys, 0 = the stream has ended
    bool dense;
};

// The chunk sequence of one workgroup; every member is uniform over the workgroup.  The tile after the current one is looked up one
// step ahead (its list entry two steps ahead), so a step never waits for a load it has just issued.
struct KeyStream {
    const int *idx, *tile_start;
    int e, e_end, id_b, s_a, c_a, cur, rem, dense_lo, dense_hi;
    bool has_a, dense, dense_pending;

    __device__ __forceinline__ int entry() {
        const int id = e < e_end ? idx[e] : -1;
        ++e;
        return id;
    }
    __device__ __forceinline__ void lookup(int id) {
        has_a = id >= 0;
        if (has_a) s_a = tile_start[id], c_a = tile_start[id + 1] - s_a;
    }
    __device__ __forceinline__ void init(const TileArgs& a, int tile, int h) {
        const int* ptr = a.nb_ptr + (a.per_head ? (int64_t)h * (a.n_tiles + 1) : 0);
        idx = a.nb_idx, tile_start = a.tile_start, e = ptr[tile], e_end = ptr[tile + 1];
        dense_lo = a.dense_lo, dense_hi = a.dense_hi, dense = false, dense_pending = true, cur = rem = 0;
        lookup(entry());
        id_b = entry();
    }
    __device__ __forceinline__ Chunk next() {
        if (rem <= 0) {
            if (has_a) {
                cur = s_a, rem = c_a;
                lookup(id_b);
                id_b = entry();
            } else if (dense_pending) {
                cur = dense_lo, rem = dense_hi - dense_lo, dense = true, dense_pending = false;
            }
        }
        Chunk c;
        c.base = cur, c.valid = rem < KVT ? (rem > 0 ? rem : 0) : KVT, c.dense = dense;
        cur += KVT, rem -= KVT;
        return c;
    }
};

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(256) void attn_tile_kernel(TileArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, g = lane >> 5;
    const int h = blockIdx.x / a.n_tiles, tile = blockIdx.x - h * a.n_tiles;    // the tiles of a head are neighbours: K/V stay in L2
    const int slot0 = a.tile_start[tile], count = a.tile_start[tile + 1] - slot0;
    const bool active = wave * 64 < count;                                       // uniform over the wave

    // Q' fragments (B operands): lane (j, g) holds channels 16 ks + 8 g .. + 7 of query slot j of each block; slots behind the count are zeros
    bf16x8 bq[2][8];
    int qrow[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int sl = wave * 64 + qb * 32 + j;
        const bool ok = sl < count;
        qrow[qb] = ok ? a.perm[slot0 + sl] : -1;
        const bf16_t* qp = a.q + (int64_t)(ok ? qrow[qb] : 0) * a.sq + h * D + g * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            float f[8];
            unpack8(ok ? *reinterpret_cast<const u32x4*>(qp + ks * 16) : u32x4{0, 0, 0, 0}, f);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = __fmul_rn(f[i], a.scale_log2e);
            bq[qb][ks] = __builtin_bit_cast(bf16x8, pack8(f));
        }
    }

    // global -> LDS: this thread's 4 keys x 8 channels of a chunk
    const int qd = lane & 15, c8 = wave * 4 + (lane >> 4);
    const bf16_t *kh = a.k + h * D + c8 * 8, *vh = a.v + h * D + c8 * 8;
    const int vt_off = KB + c8 * 8 * VP + (16 * (qd >> 2) + 8 * (qd & 1) + 4 * ((qd >> 1) & 1)) * 2;
    u32x4 stk[4], stv[4];
    auto rows_of = [&](const Chunk& c, int (&rows)[4]) {      // key rows of keys 4 qd .. 4 qd + 3, clamped to the last valid key
        if (c.valid <= 0) return;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int r = c.base + min(4 * qd + w, c.valid - 1);
            rows[w] = c.dense ? r : a.perm[r];
        }
    };
    auto fetch = [&](const int (&rows)[4]) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            stk[w] = *reinterpret_cast<const u32x4*>(kh + (int64_t)rows[w] * a.sk);
            stv[w] = *reinterpret_cast<const u32x4*>(vh + (int64_t)rows[w] * a.sv);
        }
    };
    auto stash = [&](int stage) {
        uint8_t* s = lds + stage * STAGE;
#pragma unroll
        for (int w = 0; w < 4; ++w) *reinterpret_cast<u32x4*>(s + (4 * qd + w) * KP + c8 * 16) = stk[w];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                          // word i of the four rows: channels 2 i (low halves) and 2 i + 1 (high)
            u32x2 lo, hi;
            lo[0] = (stv[0][i] & 0xffffu) | (stv[1][i] << 16), lo[1] = (stv[2][i] & 0xffffu) | (stv[3][i] << 16);
            hi[0] = (stv[0][i] >> 16) | (stv[1][i] & 0xffff0000u), hi[1] = (stv[2][i] >> 16) | (stv[3][i] & 0xffff0000u);
            *reinterpret_cast<u32x2*>(s + vt_off + (2 * i) * VP) = lo;
            *reinterpret_cast<u32x2*>(s + vt_off + (2 * i + 1) * VP) = hi;
        }
    };

    KeyStream ks;
    ks.init(a, tile, h);
    int rows[4] = {0, 0, 0, 0}, rows_next[4] = {0, 0, 0, 0};
    const Chunk c0 = ks.next();
    rows_of(c0, rows);
    const Chunk c1 = ks.next();
    rows_of(c1, rows_next);
    if (c0.valid > 0) fetch(rows), stash(0);
    if (c1.valid > 0) fetch(rows_next), stash(1);
    const Chunk c2 = ks.next();
    rows_of(c2, rows);
    int val0 = c0.valid, val1 = c1.valid, val2 = c2.valid;
    __syncthreads();

    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16 oacc[2][4];
    float m[2], l[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        m[qb] = -INFINITY, l[qb] = 0.f;
#pragma unroll
        for (int db = 0; db < 4; ++db) oacc[qb][db] = zero;
    }

    int stage = 0;
    while (val0 > 0) {                                          // chunk t in `stage`; uniform
        const Chunk c3 = ks.next();                             // slot indices of chunk t + 3
        rows_of(c3, rows_next);
        if (val2 > 0) fetch(rows);                              // rows of chunk t + 2: their indices came an iteration ago
        if (active) {
            const uint8_t* s = lds + stage * STAGE;
            f32x16 sc[2][2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    const bf16x8 ka = *reinterpret_cast<const bf16x8*>(s + (kb * 32 + j) * KP + kk * 32 + g * 16);
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb) sc[qb][kb] = mfma16(ka, bq[qb][kk], kk == 0 ? zero : sc[qb][kb]);
                }
            bf16x8 pb[2][4];
#pragma unroll
            for (int qb = 0; qb < 2; ++qb) {
                if (val0 < KVT) {                               // the last chunk of a tile or of the dense range
#pragma unroll
                    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * g >= val0) sc[qb][kb][r] = -INFINITY;
                }
                float mx = -INFINITY;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[qb][kb][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                const float mn = fmaxf(m[qb], mx);
                const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
                m[qb] = mn;
                float ls = 0.f;
#pragma unroll
                for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                    for (int hs = 0; hs < 2; ++hs) {
                        float p[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            p[e] = __builtin_amdgcn_exp2f(sc[qb][kb][hs * 8 + e] - mn);
                            ls += p[e];
                        }
                        pb[qb][kb * 2 + hs] = __builtin_bit_cast(bf16x8, pack8(p));
                    }
                l[qb] = l[qb] * alpha + ls;
                if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {      // no row of the block moved its maximum: nothing to rescale
#pragma unroll
                    for (int db = 0; db < 4; ++db) oacc[qb][db] *= alpha;
                }
            }
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int a4 = 0; a4 < 4; ++a4) {
                    const bf16x8 va = *reinterpret_cast<const bf16x8*>(s + KB + (db * 32 + j) * VP + a4 * 32 + g * 16);
#pragma unroll
                    for (int qb = 0; qb < 2; ++qb) oacc[qb][db] = mfma16(va, pb[qb][a4], oacc[qb][db]);
                }
        }
        if (val2 > 0) stash(stage == 0 ? 2 : stage - 1);        // the stage chunk t - 1 left: (t + 2) % 3
        __syncthreads();
        stage = stage == 2 ? 0 : stage + 1;
        val0 = val1, val1 = val2, val2 = c3.valid;
#pragma unroll
        for (int w = 0; w < 4; ++w) rows[w] = rows_next[w];
    }

    // epilogue: the two halves g of a query column share its row; O / l as bf16, four channels (8 bytes) a store
    if (!active) return;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const float lt = l[qb] + __shfl_xor(l[qb], 32, 64);
        const float inv = lt > 0.f ? 1.0f / lt : 0.f;
        if (qrow[qb] >= 0) {
            bf16_t* orow = a.o + (int64_t)qrow[qb] * a.so + h * D;
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    u32x2 w;
                    w[0] = pack_bf2(oacc[qb][db][r4 * 4] * inv, oacc[qb][db][r4 * 4 + 1] * inv);
                    w[1] = pack_bf2(oacc[qb][db][r4 * 4 + 2] * inv, oacc[qb][db][r4 * 4 + 3] * inv);
                    *reinterpret_cast<u32x2*>(orow + db * 32 + r4 * 8 + g * 4) = w;
                }
        }
    }
}

}  // namespace

extern "C" int hv_attn_fwd_tile_bf16(const void* q, const void* k, const void* v, void* o, int64_t stride_q, int64_t stride_k,
                                     int64_t stride_v, int64_t stride_o, int n_q, int n_kv, int n_heads, int head_dim, float scale,
                                     const int* perm, const int* tile_start, int n_tiles, const int* nb_ptr, const int* nb_idx, int n_lists,
                                     int dense_lo, int dense_hi, hipStream_t stream) {
    if (!q || !k || !v || !o || !perm || !tile_start || !nb_ptr || !nb_idx || head_dim != D || n_heads <= 0 || n_heads > 65535 ||
        n_q < 0 || n_kv < n_q || n_kv > MAX_KV || n_tiles <= 0 || (n_lists != 1 && n_lists != n_heads) || dense_lo < 0 ||
        dense_lo > dense_hi || dense_hi > n_kv || (stride_q & 7) || (stride_k & 7) || (stride_v & 7) || (stride_o & 3) ||
        !hv_pitch_ok(n_q, stride_o, (int64_t)n_heads * D) || !hv_grid_x_ok((int64_t)n_tiles * n_heads))
        return HV_ERR_ARG;
    if (n_q == 0) return HV_OK;
    if (n_tiles > n_q) return HV_ERR_ARG;
    static HvPerDeviceOnce once;
    TileArgs a;
    a.q = (const bf16_t*)q, a.k = (const bf16_t*)k, a.v = (const bf16_t*)v, a.o = (bf16_t*)o;
    a.sq = stride_q, a.sk = stride_k, a.sv = stride_v, a.so = stride_o;
    a.perm = perm, a.tile_start = tile_start, a.nb_ptr = nb_ptr, a.nb_idx = nb_idx;
    a.n_tiles = n_tiles, a.per_head = n_lists != 1, a.dense_lo = dense_lo, a.dense_hi = dense_hi;
    a.scale_log2e = scale * 1.4426950408889634f;
    if (hv_set_max_lds(once, (const void*)attn_tile_kernel, LDS_BYTES) != HV_OK) return HV_ERR_LAUNCH;
    attn_tile_kernel<<<dim3((unsigned)(n_tiles * n_heads)), dim3(256), LDS_BYTES, stream>>>(a);
    return hv_check_launch();
}
