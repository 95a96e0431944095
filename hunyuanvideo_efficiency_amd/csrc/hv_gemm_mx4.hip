// MXFP4 linears (opt-in; include/hv_gemm_mx4.h holds the format contract): the block-scaled e2m1 GEMM on
// v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 4: both operands FP4, E8M0 block scales applied inside the matrix pipe) and the
// two quantisers that produce its operands.
//
// GEMM main loop, one workgroup (8 waves, 2 along M x 4 along N) per 256 x 256 outputs, a wave 128 x 64 = 8 x 4 accumulators:
//   * a K-stage is 128 k = ONE matrix instruction per accumulator.  Per operand it is 256 rows x 64 bytes = 16 KiB, moved HBM -> LDS
//     by two global_load_lds_dwordx4 per thread; a lane's whole 32-k operand is one 16-byte chunk = one ds_read_b128 into 4 VGPRs,
//     and those 32 k are exactly one scale block.  LDS rows are 64 bytes; chunk c of row r sits at chunk position c ^ ((r >> 2) & 3)
//     (applied on the DMA's source address and on the read), so the 16 lanes of a read that share a k-block hit 16 different
//     16-byte bank groups.
//   * W rows are dealt to LDS rows so that the 16 MFMA rows of n-repeat ni are 16 consecutive LDS rows (the same read formula as A)
//     and hold W rows (ni >> 1) * 32 + (i >> 2) * 8 + (ni & 1) * 4 + (i & 3): issued as D = W . A^T, a lane then owns 8 consecutive n
//     of one m per pair of n-repeats -> 16-byte bf16 stores, the epilogue shape of hv_gemm.hip.
//   * scales: per stage a row has 4 scale bytes (its 4 k-blocks) = one aligned dword, loaded by thread = row (waves 0-3: the 256 A
//     rows, waves 4-7: the 256 W rows) and written to LDS byte by byte, TRANSPOSED: dword (16-row-group quad, k-block, row in group)
//     collects, in its 4 bytes, the scales of four 16-row groups.  A lane reads the dword of (its k-block, its row) - conflict-free
//     ds_read_b32, two for A (m-repeats 0-3, 4-7), one for W (n-repeats 0-3) - and the instruction's op_sel picks the byte: one
//     register serves four matrix instructions, no VALU unpacking.  (Row-major scale dwords in LDS would cost 12 reads and 12
//     lane-variable shifts per stage instead of 3 reads.)
//   * ring of 4 slots x 34 KiB = 136 KiB; registers: two sets of W fragments (stage t, t + 1) and two sets of four A fragments (an
//     m-half each).  Iteration t: read A half 1 of stage t, issue the DMA + scale load of stage t + 3 (into the slot stage t - 1 left
//     at the last barrier), 16 matrix instructions on half 0, read W and A half 0 of stage t + 1, 16 instructions on half 1, wait
//     with a counted vmcnt for the thread's own loads of stage t + 2 and store its scale bytes, barrier.  A stage is read one
//     barrier after the wait that retired it; a slot is re-filled one barrier after its last read.
// Both compiler hazards noted in hv_gemm.hip apply (same intrinsic): after the loop every accumulator is pinned under the full
// EXEC mask and the epilogue's pointers are made opaque, so neither a matrix instruction sinks into a masked region nor an epilogue
// load rises into the counted waits.
#include "hv_common.hpp"
#include "hv_ln_row.hpp"
#include "hv_mx4_quant.hpp"
#include "hv_mx_tile.hpp"
#include "hv_tile_order.hpp"
#include "../../include/hv_gemm_mx4.h"

namespace {

constexpr int BM = HV_MX4_BM, BN = HV_MX4_BN, KS = HV_MX4_KSTAGE, RING = HV_MX4_RING;
constexpr int OP_BYTES = 256 * (KS / 2);             // one operand of one stage: 16 KiB
constexpr int SC_BYTES = 256 * (KS / 32);            // its scales: 1 KiB
constexpr int SLOT_BYTES = 2 * OP_BYTES + 2 * SC_BYTES;
constexpr int LDS_BYTES = RING * SLOT_BYTES;         // 136 KiB
constexpr int OPS_PER_STAGE = 5;                     // vector-memory operations a thread issues per stage: 4 DMA + 1 scale dword

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

using Mx4Args = MxGemmArgs;        // hv_mx_tile.hpp: argument block, W row deal and epilogue shared with hv_gemm_mx6.hip

// one scaled FP4 matrix instruction: 4-register operands travel in the low half of the builtin's 8-register type (cbsz = blgp = 4
// makes the instruction read 4); OW / OA = byte of the scale register (op_sel), an immediate
template <int OW, int OA>
__device__ __forceinline__ f32x4 mfma_mx4(i32x4 w, int sw, i32x4 a, int sa, f32x4 c) {
    const i32x4 z = {0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_shufflevector(w, z, 0, 1, 2, 3, 4, 5, 6, 7),
                                                            __builtin_shufflevector(a, z, 0, 1, 2, 3, 4, 5, 6, 7), c, 4, 4, OW, sw, OA, sa);
}

__global__ __launch_bounds__(512, 2) void gemm_mx4_kernel(Mx4Args g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fq = lane >> 4;

    const TileMN tile = tile_of(xcd_linear_tile(), g.tiles_m, g.tiles_n);
    const int m0 = tile.tm * BM, n0 = tile.tn * BN;

    // ---- staging.  Codes: piece i of an operand = LDS rows [i * 128, i * 128 + 128), thread -> (row i * 128 + (tid >> 2), chunk
    // position tid & 3), which holds chunk (tid & 3) ^ ((row >> 2) & 3) of the row.  Tails read clamped (valid) rows.
    uint32_t a_o[2], w_o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int lr = i * 128 + (tid >> 2);
        const uint32_t chunk = (uint32_t)(((tid & 3) ^ ((lr >> 2) & 3)) << 4);
        a_o[i] = (uint32_t)((int64_t)(min(m0 + lr, g.M - 1) - m0) * g.lda) + chunk;
        w_o[i] = (uint32_t)((int64_t)(min(n0 + w_tile_row(lr), g.N - 1) - n0) * g.ldw) + chunk;
    }
    const char* a_tile = reinterpret_cast<const char*>(g.A) + (int64_t)m0 * g.lda;
    const char* w_tile = reinterpret_cast<const char*>(g.W) + (int64_t)n0 * g.ldw;
    // Scales: thread = row.  Waves 0-3: A tile row tid; waves 4-7: LDS W row tid - 256.  sc_dst = byte address (inside a slot's
    // scale area) of the row's k-block 0; k-block kb is 64 bytes (16 dwords) further.
    const int srow = tid & 255;
    const bool sc_is_w = wave >= 4;           // wave-uniform
    const char* sc_tile = sc_is_w ? reinterpret_cast<const char*>(g.Ws) + (int64_t)n0 * g.ldws
                                  : reinterpret_cast<const char*>(g.As) + (int64_t)m0 * g.ldas;
    const uint32_t sc_o = sc_is_w ? (uint32_t)((int64_t)(min(n0 + w_tile_row(srow), g.N - 1) - n0) * g.ldws)
                                  : (uint32_t)((int64_t)(min(m0 + srow, g.M - 1) - m0) * g.ldas);
    // A: dword ((row >> 6) * 64 + kb * 16 + (row & 15)), byte (row >> 4) & 3 [row >> 6 = wm * 2 + h];  W: dword (wn * 64 + kb * 16 + i), byte ni
    const int sc_dst = 2 * OP_BYTES + (sc_is_w ? SC_BYTES : 0) + ((srow >> 6) * 64 + (srow & 15)) * 4 + ((srow >> 4) & 3);

    // every source is a wave-uniform base kept a scalar pair (the asm stops the compiler folding it into per-lane 64-bit pointers) plus
    // an invariant 32-bit per-lane offset: the saddr + voffset form, no 64-bit vector arithmetic in the loop
    auto opaque = [](const char* p) {
        uint64_t v = reinterpret_cast<uint64_t>(p);
        asm volatile("" : "+s"(v));
        return reinterpret_cast<const char*>(v);
    };
    auto issue = [&](int stage, uint32_t& sreg) {       // DMA of the stage's codes + the row's scale dword into a register
        char* dst = smem + (stage & (RING - 1)) * SLOT_BYTES + wave * 1024;
        const char* as = opaque(a_tile + stage * (KS / 2));
        const char* ws = opaque(w_tile + stage * (KS / 2));
        const char* ss = opaque(sc_tile + stage * (KS / 32));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t o = a_o[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(as + o), (lds_ptr_t)(dst + i * 8192), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t o = w_o[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ws + o), (lds_ptr_t)(dst + OP_BYTES + i * 8192), 16, 0, 0);
        }
        uint32_t o = sc_o;
        asm volatile("" : "+v"(o));
        sreg = *(const __attribute__((address_space(1))) uint32_t*)(ss + o);      // (a global, not a flat, load: the asm hid the address space)
    };
    // (the four byte stores are written as asm: for a compiler-visible LDS store the compiler first drains EVERY LDS-DMA in flight -
    // it cannot tell that the scale area is never a DMA target - which would empty the ring once per stage.  The s_waitcnt lgkmcnt(0)
    // before the stage's barrier covers them.)
    auto put_scales = [&](int stage, uint32_t sreg) {
        const uint32_t dst = (uint32_t)(uintptr_t)(lds_ptr_t)(smem + (stage & (RING - 1)) * SLOT_BYTES + sc_dst);
        asm volatile("ds_write_b8 %0, %1\n\tds_write_b8 %0, %2 offset:64\n\tds_write_b8 %0, %3 offset:128\n\tds_write_b8 %0, %4 offset:192"
                     : : "v"(dst), "v"(sreg), "v"(sreg >> 8), "v"(sreg >> 16), "v"(sreg >> 24) : "memory");
    };

    // ---- fragments: lane (fr, fq) reads chunk fq of row (16-row group base + fr).  Registers: two sets of W fragments (stage t and
    // t + 1) and two sets of FOUR A fragments (an m-half each): 64 VGPRs beside the 128 accumulators.
    const int frag_rd = fr * 64 + ((fq ^ (fr >> 2)) << 4);
    const int a_rd = wm * 128 * 64 + frag_rd;                 // + mi * 1024
    const int w_rd = OP_BYTES + wn * 64 * 64 + frag_rd;       // + ni * 1024
    const int sa_rd = 2 * OP_BYTES + (wm * 128 + lane) * 4;   // + h * 256
    const int sw_rd = 2 * OP_BYTES + SC_BYTES + (wn * 64 + lane) * 4;
    i32x4 ah[2][4], wf[2][4];
    int sa[2], sw[2];
    auto read_w = [&](auto Pc, int stage) {
        constexpr int P = decltype(Pc)::value;
        const char* base = smem + (stage & (RING - 1)) * SLOT_BYTES;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) wf[P][ni] = *reinterpret_cast<const i32x4*>(base + w_rd + ni * 1024);
        sw[P] = *reinterpret_cast<const int*>(base + sw_rd);
    };
    auto read_a = [&](auto Hc, int stage) {       // m-repeats 4 H .. 4 H + 3
        constexpr int H = decltype(Hc)::value;
        const char* base = smem + (stage & (RING - 1)) * SLOT_BYTES;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) ah[H][mi] = *reinterpret_cast<const i32x4*>(base + a_rd + (4 * H + mi) * 1024);
        sa[H] = *reinterpret_cast<const int*>(base + sa_rd + H * 256);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](auto Pc, auto Hc) {            // 16 matrix instructions: m-half H against the stage's four W fragments
        constexpr int P = decltype(Pc)::value, H = decltype(Hc)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        static_for(std::make_integer_sequence<int, 4>{}, [&](auto mic) {
            constexpr int mi = decltype(mic)::value;
            static_for(std::make_integer_sequence<int, 4>{}, [&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                acc[4 * H + mi][ni] = mfma_mx4<ni, mi>(wf[P][ni], sw[P], ah[H][mi], sa[H], acc[4 * H + mi][ni]);
            });
        });
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const int nkt = g.K / KS;          // >= 4 (host side)
    // Register set of stage t: (t + par) & 1 with par = nkt & 1, so that the four tail iterations always see sets (0, 1, 0, 1): an
    // odd stage count is absorbed by ONE peeled iteration in front, not by a second copy of the tail.
    const int par = nkt & 1;
    uint32_t sreg[2], s0, s1, s2;
    // ---- prologue: stages 0, 1, 2 in flight, all of it landed (one exposed latency per tile), scales of 0 and 1 stored; stage 2's
    // scale dword waits in the register the first iteration stores from (either parity: both hold it)
    issue(0, s0);
    issue(1, s1);
    issue(2, s2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    put_scales(0, s0);
    put_scales(1, s1);
    sreg[0] = sreg[1] = s2;
    __syncthreads();
    if (par) read_w(I1{}, 0);
    else read_w(I0{}, 0);
    read_a(I0{}, 0);

    // R = min(nkt - t, 4), the stages left including this one, is a compile-time constant: the steady loop (R = 4) and the seven
    // tail iterations have no branches, and every vmcnt is a literal
    auto step = [&](auto Pc, auto Rc, int t) {
        constexpr int P = decltype(Pc)::value, R = decltype(Rc)::value;
        using Q = std::integral_constant<int, P ^ 1>;
        read_a(I1{}, t);
        if constexpr (R > 3) issue(t + 3, sreg[P]);
        mma(Pc, I0{});
        if constexpr (R > 1) {
            read_w(Q{}, t + 1);
            read_a(I0{}, t + 1);
        }
        mma(Pc, I1{});
        if constexpr (R > 2) {
            // the thread's own loads of stage t + 2 are older than the OPS_PER_STAGE of stage t + 3 (if that was issued)
            asm volatile("s_waitcnt vmcnt(%0)" : : "n"(R > 3 ? OPS_PER_STAGE : 0) : "memory");
            put_scales(t + 2, sreg[P ^ 1]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using I4 = std::integral_constant<int, 4>;
    int t = 0;
    if (par) {                              // nkt odd, so >= 5: stage 3 exists
        step(I1{}, I4{}, 0);
        t = 1;
    }
    for (; t + 4 < nkt; t += 2) {           // t + 1 + 3 < nkt; leaves nkt - t == 4
        step(I0{}, I4{}, t);
        step(I1{}, I4{}, t + 1);
    }
    step(I0{}, I4{}, t);
    step(I1{}, I3{}, t + 1);
    step(I0{}, I2{}, t + 2);
    step(I1{}, I1{}, t + 3);

    // ---- hand-off: accumulators pinned under the full EXEC mask, epilogue pointers opaque (see the header comment)
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) asm volatile("" : : "v"(acc[mi][ni]));
    Mx4Args ge = g;
    asm volatile("s_waitcnt vmcnt(0)" : "+s"(ge.bias), "+s"(ge.gate), "+s"(ge.res), "+s"(ge.out0), "+s"(ge.out1) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    mx_epilogue(ge, acc, m0 + wm * 128 + fr, n0 + wn * 64, fq);
}

// ------------------------------------------------------------------------------------------------ quantisers
// (the rule itself - e2m1_code, mx4_quant8 - lives in hv_mx4_quant.hpp, shared with the rotated quantisers of hv_mx_rot.hip)
__global__ __launch_bounds__(256) void quant_rows_mx4_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ codes,
                                                              int64_t ldq, uint8_t* __restrict__ scales, int64_t lds, int64_t M, int K) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bf16_t* xr = x + row * ldx;
    const int nchunk = K >> 3;              // a multiple of 4: the four lanes of a block run the same trips
    for (int ch = lane; ch < nchunk; ch += 64) {
        float f[8];
        unpack8(*reinterpret_cast<const u32x4*>(xr + ch * 8), f);
        uint32_t e;
        const uint32_t w = mx4_quant8(f, e);
        *reinterpret_cast<uint32_t*>(codes + row * ldq + ch * 4) = w;
        if ((lane & 3) == 0) scales[row * lds + (ch >> 2)] = (uint8_t)e;
    }
}

// hv_ln_modulate_bf16 mode 0 up to the bf16 rounding (ln_mod_kernel's statistics and coefficients), then the quantiser
template <int MAXC>
__global__ __launch_bounds__(256) void ln_mod_mx4_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ add,
                                                          const bf16_t* __restrict__ mul, uint8_t* __restrict__ codes, int64_t ldq,
                                                          uint8_t* __restrict__ scales, int64_t lds, int64_t M, int D, int64_t ldx,
                                                          float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int nchunk = D >> 3;
    float v[MAXC][8];
    const float mean = wave_sum(ln_load_row<MAXC>(x + row * ldx, lane, nchunk, v)) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float d = v[c][j] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + c * 64;
        if (ch < nchunk) {                  // nchunk % 4 == 0: taken by whole blocks of four lanes
            float m[8], a[8];
            ln_load_coeffs(mul, add, ch, 0, m, a);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = rbf((v[c][j] - mean) * rstd * m[j] + a[j]);
            uint32_t e;
            const uint32_t w = mx4_quant8(v[c], e);
            *reinterpret_cast<uint32_t*>(codes + row * ldq + ch * 4) = w;
            if ((lane & 3) == 0) scales[row * lds + (ch >> 2)] = (uint8_t)e;
        }
    }
}

}  // namespace

extern "C" int hv_quant_rows_mxfp4(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, int64_t M, int K,
                                   hipStream_t stream) {
    if (!mx4_quant_args_ok(x, codes, scales, M, K, ldx, ldq, lds)) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    quant_rows_mx4_kernel<<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream>>>((const bf16_t*)x, ldx, (uint8_t*)codes, ldq,
                                                                                  (uint8_t*)scales, lds, M, K);
    return hv_check_launch();
}

extern "C" int hv_ln_modulate_mxfp4(const void* x, const void* shift, const void* scale, void* codes, int64_t ldq, void* scales,
                                    int64_t lds, int64_t M, int D, int64_t ldx, float eps, hipStream_t stream) {
    if (!mx4_quant_args_ok(x, codes, scales, M, D, ldx, ldq, lds) || D > 4096) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    dim3 grid((unsigned)((M + 3) / 4)), block(256);
    ln_dispatch_maxc(D, [&](auto maxc) {
        ln_mod_mx4_kernel<decltype(maxc)::value><<<grid, block, 0, stream>>>((const bf16_t*)x, (const bf16_t*)shift, (const bf16_t*)scale,
                                                                             (uint8_t*)codes, ldq, (uint8_t*)scales, lds, M, D, ldx, eps);
    });
    return hv_check_launch();
}

extern "C" int hv_gemm_mxfp4(const void* A_codes, int64_t lda, const void* A_scales, int64_t ldas, const void* W_codes, int64_t ldw,
                             const void* W_scales, int64_t ldws, const void* bias, int M, int N, int K, void* out0, int64_t ld0, int act0,
                             int n_split, void* out1, int64_t ld1, int act1, const void* gate, const void* res, int64_t ld_res,
                             hipStream_t stream) {
    Mx4Args g{};
    if (K < HV_MX4_MIN_K || (K % KS) || !mx_gemm_args(g, A_codes, lda, A_scales, ldas, W_codes, ldw, W_scales, ldws, bias, M, N, K, out0, ld0, act0,
                                                     n_split, out1, ld1, act1, gate, res, ld_res))
        return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    static HvPerDeviceOnce once;
    if (hv_set_max_lds(once, (const void*)gemm_mx4_kernel, LDS_BYTES) != HV_OK) return HV_ERR_LAUNCH;
    gemm_mx4_kernel<<<dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(512), LDS_BYTES, stream>>>(g);
    return hv_check_launch();
}
