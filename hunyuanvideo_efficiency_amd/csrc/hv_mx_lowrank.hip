// MXFP4 linears with a low-rank bf16 branch (opt-in; include/hv_mx_lowrank.h holds the contract): y = Q4(A) Q4(Res)^T + T Up^T with
// T = bf16(A Dn^T), as two kernels - the GEMM with the rank-R product folded into its accumulators, and the activation pass that
// produces T while it quantises.
//
// GEMM.  gemm_mx4_kernel's work split and ring (hv_gemm_mx4.hip: 256 x 256 outputs, 8 waves, K-stages of 128 codes = 256 rows x 64
// bytes per operand, four slots filled by global_load_lds_dwordx4 three stages ahead, one barrier per stage) with RS = R / 32 rank
// stages in FRONT of the K / 128 code stages.  A rank stage is 32 bf16 of T / Up per row = the same 256 rows x 64 bytes, dealt, swizzled
// and read exactly like a code stage: lane (fr, fq) reads 16-byte chunk fq of row fr, which is k-block fq for the FP4 instruction and
// k = 8 fq .. 8 fq + 7 for v_mfma_f32_16x16x32_bf16, and both write D alike.  So a rank stage differs in three places only: its DMA
// sources (T, Up and no scale dword: 4 vector-memory operations instead of 5, which the counted vmcnt of the stage before it has to
// know), the instruction, and the scale bytes it neither stores nor uses (read_w / read_a still fetch the slot's idle scale dwords:
// never consumed).  The rank stages are stages 0 .. RS - 1 of the ring, run by RS peeled iterations; the kernel is instantiated per RS, so
// which of stages t + 2 and t + 3 is a rank stage is known at compile time and every vmcnt stays a literal; from stage RS on the loop is hv_gemm_mxfp4's: steady body and compile-time tail without a branch.  The
// register-set parity counts all K / 128 + RS stages, so the tail still sees sets (0, 1, 0, 1).
//
// Quantise + down-project.  A workgroup of 8 waves owns 128 rows and walks K in chunks of 128: the x band (128 x 256 bytes) and R rows
// of Dn (R x 256 bytes) stand side by side in LDS at a row pitch of 272 bytes, which spreads the 16 rows of a 16-byte fragment read over
// all 64 banks.  The next chunk is loaded into registers (16-byte coalesced loads, a row's 256 bytes by 16 adjacent lanes) before this
// one is used and stored to LDS after it.  Per 32 k a wave reads ONE x fragment - lane (fr, fq): k 8 fq .. 8 fq + 7 of its row fr -
// which is the B operand of R / 16 matrix instructions (D = Dn . x^T: a lane ends with 4 consecutive j of row fr, an 8-byte T store)
// and a quarter of the row's MX block; the block maximum crosses lanes fr, fr + 16, fr + 32, fr + 48, then mx4_codes8.
// Built without the packed fp32 instructions like hv_gemm_mx4.hip (Makefile): codes and scales are pinned bit for bit.
#include "hv_common.hpp"
#include "hv_mx4_quant.hpp"
#include "hv_mx_tile.hpp"
#include "hv_tile_order.hpp"
#include "../../include/hv_mx_lowrank.h"

namespace {

constexpr int BM = HV_MX4_BM, BN = HV_MX4_BN, KS = HV_MX4_KSTAGE, RING = HV_MX4_RING, RC = HV_MX_LR_CHUNK;
constexpr int OP_BYTES = 256 * (KS / 2);             // one operand of one stage: 16 KiB (code stage: 128 codes, rank stage: 32 bf16 a row)
constexpr int SC_BYTES = 256 * (KS / 32);
constexpr int SLOT_BYTES = 2 * OP_BYTES + 2 * SC_BYTES;
constexpr int LDS_BYTES = RING * SLOT_BYTES;         // 136 KiB
constexpr int OPS_CODE = 5, OPS_RANK = 4;            // vector-memory operations a thread issues per stage (4 DMA + the scale dword)
static_assert(RC * 2 == KS / 2, "a rank stage must be as many bytes per row as a code stage");

typedef __attribute__((ext_vector_type(4))) int i32x4;

struct LrGemmArgs {
    MxGemmArgs g;
    const uint16_t *T, *Up;
    int64_t ldt, ldu;
};

template <int OW, int OA>
__device__ __forceinline__ f32x4 mfma_mx4(i32x4 w, int sw, i32x4 a, int sa, f32x4 c) {
    const i32x4 z = {0, 0, 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_shufflevector(w, z, 0, 1, 2, 3, 4, 5, 6, 7),
                                                            __builtin_shufflevector(a, z, 0, 1, 2, 3, 4, 5, 6, 7), c, 4, 4, OW, sw, OA, sa);
}
__device__ __forceinline__ f32x4 mfma_bf16(i32x4 w, i32x4 a, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
}

template <int RS>                          // R / 32 = 1 .. 4: which of the first stages are rank stages is known at compile time
__global__ __launch_bounds__(512, 2) void gemm_mx4_lr_kernel(LrGemmArgs q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const MxGemmArgs& g = q.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fq = lane >> 4;

    const TileMN tile = tile_of(xcd_linear_tile(), g.tiles_m, g.tiles_n);
    const int m0 = tile.tm * BM, n0 = tile.tn * BN;

    // ---- staging, as gemm_mx4_kernel: piece i of an operand = LDS rows [i * 128, i * 128 + 128), thread -> (row i * 128 + (tid >> 2),
    // chunk position tid & 3) holding chunk (tid & 3) ^ ((row >> 2) & 3).  The rank operands take the same rows and chunks of T / Up
    // (a bf16 row pitch is 2 ldt / 2 ldu bytes); their offsets are worked out where they are used, at most four times a tile, so that
    // they hold no registers beside the 237 of gemm_mx4_kernel.  Tails read clamped (valid) rows.
    auto offsets = [&](uint32_t (&ao)[2], int64_t a_pitch, uint32_t (&wo)[2], int64_t w_pitch) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int lr = i * 128 + (tid >> 2);
            const uint32_t chunk = (uint32_t)(((tid & 3) ^ ((lr >> 2) & 3)) << 4);
            ao[i] = (uint32_t)((int64_t)(min(m0 + lr, g.M - 1) - m0) * a_pitch) + chunk;
            wo[i] = (uint32_t)((int64_t)(min(n0 + w_tile_row(lr), g.N - 1) - n0) * w_pitch) + chunk;
        }
    };
    uint32_t a_o[2], w_o[2];
    offsets(a_o, g.lda, w_o, g.ldw);
    const char* a_tile = reinterpret_cast<const char*>(g.A) + (int64_t)m0 * g.lda;
    const char* w_tile = reinterpret_cast<const char*>(g.W) + (int64_t)n0 * g.ldw;
    const char* t_tile = reinterpret_cast<const char*>(q.T) + (int64_t)m0 * q.ldt * 2;
    const char* u_tile = reinterpret_cast<const char*>(q.Up) + (int64_t)n0 * q.ldu * 2;
    const int srow = tid & 255;
    const bool sc_is_w = wave >= 4;           // wave-uniform
    const char* sc_tile = sc_is_w ? reinterpret_cast<const char*>(g.Ws) + (int64_t)n0 * g.ldws
                                  : reinterpret_cast<const char*>(g.As) + (int64_t)m0 * g.ldas;
    const uint32_t sc_o = sc_is_w ? (uint32_t)((int64_t)(min(n0 + w_tile_row(srow), g.N - 1) - n0) * g.ldws)
                                  : (uint32_t)((int64_t)(min(m0 + srow, g.M - 1) - m0) * g.ldas);
    const int sc_dst = 2 * OP_BYTES + (sc_is_w ? SC_BYTES : 0) + ((srow >> 6) * 64 + (srow & 15)) * 4 + ((srow >> 4) & 3);

    auto opaque = [](const char* p) {
        uint64_t v = reinterpret_cast<uint64_t>(p);
        asm volatile("" : "+s"(v));
        return reinterpret_cast<const char*>(v);
    };
    // the four DMAs of a stage: 64 bytes a row of each operand, from sources already advanced to the stage's columns
    auto dma = [&](int stage, const char* a_src, const uint32_t (&ao)[2], const char* w_src, const uint32_t (&wo)[2]) {
        char* dst = smem + (stage & (RING - 1)) * SLOT_BYTES + wave * 1024;
        const char* as = opaque(a_src);
        const char* ws = opaque(w_src);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t o = ao[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(as + o), (lds_ptr_t)(dst + i * 8192), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            uint32_t o = wo[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ws + o), (lds_ptr_t)(dst + OP_BYTES + i * 8192), 16, 0, 0);
        }
    };
    auto issue_rank = [&](int stage) {                                                                               // stage < RS
        uint32_t t_o[2], u_o[2];
        offsets(t_o, q.ldt * 2, u_o, q.ldu * 2);
        dma(stage, t_tile + stage * (RC * 2), t_o, u_tile + stage * (RC * 2), u_o);
    };
    auto issue_code = [&](int stage, uint32_t& sreg) {                                                               // stage >= RS
        const int ks = stage - RS;
        dma(stage, a_tile + ks * (KS / 2), a_o, w_tile + ks * (KS / 2), w_o);
        const char* ss = opaque(sc_tile + ks * (KS / 32));
        uint32_t o = sc_o;
        asm volatile("" : "+v"(o));
        sreg = *(const __attribute__((address_space(1))) uint32_t*)(ss + o);
    };
    // (asm stores: see gemm_mx4_kernel - a compiler-visible LDS store would drain every LDS-DMA in flight)
    auto put_scales = [&](int stage, uint32_t sreg) {
        const uint32_t dst = (uint32_t)(uintptr_t)(lds_ptr_t)(smem + (stage & (RING - 1)) * SLOT_BYTES + sc_dst);
        asm volatile("ds_write_b8 %0, %1\n\tds_write_b8 %0, %2 offset:64\n\tds_write_b8 %0, %3 offset:128\n\tds_write_b8 %0, %4 offset:192"
                     : : "v"(dst), "v"(sreg), "v"(sreg >> 8), "v"(sreg >> 16), "v"(sreg >> 24) : "memory");
    };

    // ---- fragments: lane (fr, fq) reads chunk fq of row (16-row group base + fr), for either kind of stage
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
    auto read_a = [&](auto Sc, auto Hc, int stage) {       // m-repeats 4 H .. 4 H + 3 into register set S
        constexpr int S = decltype(Sc)::value, H = decltype(Hc)::value;
        const char* base = smem + (stage & (RING - 1)) * SLOT_BYTES;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) ah[S][mi] = *reinterpret_cast<const i32x4*>(base + a_rd + (4 * H + mi) * 1024);
        sa[S] = *reinterpret_cast<const int*>(base + sa_rd + H * 256);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    // 16 matrix instructions: m-half H, held in A register set S, against the W fragments of set P; LEAD = a rank stage (bf16, unscaled)
    auto mma = [&](auto Pc, auto Sc, auto Hc, auto Lc) {
        constexpr int P = decltype(Pc)::value, S = decltype(Sc)::value, H = decltype(Hc)::value;
        constexpr bool LEAD = decltype(Lc)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        static_for(std::make_integer_sequence<int, 4>{}, [&](auto mic) {
            constexpr int mi = decltype(mic)::value;
            static_for(std::make_integer_sequence<int, 4>{}, [&](auto nic) {
                constexpr int ni = decltype(nic)::value;
                if constexpr (LEAD) acc[4 * H + mi][ni] = mfma_bf16(wf[P][ni], ah[S][mi], acc[4 * H + mi][ni]);
                else acc[4 * H + mi][ni] = mfma_mx4<ni, mi>(wf[P][ni], sw[P], ah[S][mi], sa[S], acc[4 * H + mi][ni]);
            });
        });
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const int nkt = g.K / KS;          // >= 4 (host side)
    const int nst = nkt + RS;
    // Register set of code stage t: (t - RS + par) & 1 with par = nkt & 1, so that the four tail iterations always see sets (0, 1, 0, 1).
    // The rank stages take no part in that: they run out of set 0 alone (below).
    const int par = nkt & 1;
    uint32_t sreg[2] = {0, 0}, lreg[2] = {0, 0}, s1 = 0, s2 = 0;
    // ---- prologue: stages 0, 1, 2 in flight and landed; stage 0 is a rank stage, 1 and 2 are where RS says so.  The scales of a code
    // stage 1 are stored here, those of a code stage 2 wait in s2 for the first iteration
    issue_rank(0);
    if constexpr (RS > 1) issue_rank(1);
    else issue_code(1, s1);
    if constexpr (RS > 2) issue_rank(2);
    else issue_code(2, s2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (RS == 1) put_scales(1, s1);
    __syncthreads();
    read_w(I0{}, 0);
    read_a(I0{}, I0{}, 0);

    // The peeled iteration of rank stage T: the ring moves as in every iteration (stage T + 3 issued - of either kind, its operation
    // count the literal of the vmcnt - and stage T + 2 retired, with scales to store if it is a code stage), but the fragments are
    // NOT double-buffered: W in set 0, both m-halves through A set 0, the next stage's fragments read after the last instruction.
    // That leaves 32 registers free where the accumulators are first written, which keeps these iterations out of scratch, and
    // exposes two LDS round trips in each of the R / 32 rank iterations of a tile (the SIMD's other wave fills them).  The last one
    // reads W of the first code stage into the set its parity asks for.  Scale dwords in flight: a rank iteration keeps them in lreg
    // (stage 2's is s2), except the last one, whose stage T + 3 is retired by the first code iteration out of sreg[par ^ 1].
    auto lead_step = [&](auto Tc) {
        constexpr int T = decltype(Tc)::value;
        if constexpr (T + 3 < RS) issue_rank(T + 3);
        else if constexpr (T + 1 < RS) issue_code(T + 3, lreg[T & 1]);
        else if (par) issue_code(T + 3, sreg[0]);
        else issue_code(T + 3, sreg[1]);
        mma(I0{}, I0{}, I0{}, std::true_type{});
        read_a(I0{}, I1{}, T);
        mma(I0{}, I0{}, I1{}, std::true_type{});
        if constexpr (T + 1 < RS) read_w(I0{}, T + 1);
        else if (par) read_w(I1{}, T + 1);
        else read_w(I0{}, T + 1);
        read_a(I0{}, I0{}, T + 1);
        asm volatile("s_waitcnt vmcnt(%0)" : : "n"(T + 3 < RS ? OPS_RANK : OPS_CODE) : "memory");
        if constexpr (T + 2 >= RS) put_scales(T + 2, T == 0 ? s2 : lreg[(T & 1) ^ 1]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    // gemm_mx4_kernel's iteration on code stage t: R = min(nst - t, 4) stages left including this one
    auto step = [&](auto Pc, auto Rc, int t) {
        constexpr int P = decltype(Pc)::value, R = decltype(Rc)::value;
        using Q = std::integral_constant<int, P ^ 1>;
        read_a(I1{}, I1{}, t);
        if constexpr (R > 3) issue_code(t + 3, sreg[P]);
        mma(Pc, I0{}, I0{}, std::false_type{});
        if constexpr (R > 1) {
            read_w(Q{}, t + 1);
            read_a(I0{}, I0{}, t + 1);
        }
        mma(Pc, I1{}, I1{}, std::false_type{});
        if constexpr (R > 2) {
            // the thread's own loads of stage t + 2 are older than the OPS_CODE of stage t + 3 (if that was issued)
            asm volatile("s_waitcnt vmcnt(%0)" : : "n"(R > 3 ? OPS_CODE : 0) : "memory");
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
    static_for(std::make_integer_sequence<int, RS>{}, [&](auto tc) { lead_step(tc); });
    int t = RS;
    if (par) {                              // K / 128 odd, so >= 5: stage t + 3 exists
        step(I1{}, I4{}, t);
        ++t;
    }
    for (; t + 4 < nst; t += 2) {           // leaves nst - t == 4
        step(I0{}, I4{}, t);
        step(I1{}, I4{}, t + 1);
    }
    step(I0{}, I4{}, t);
    step(I1{}, I3{}, t + 1);
    step(I0{}, I2{}, t + 2);
    step(I1{}, I1{}, t + 3);

    // ---- hand-off: accumulators pinned under the full EXEC mask, epilogue pointers opaque (see hv_gemm_mx4.hip)
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) asm volatile("" : : "v"(acc[mi][ni]));
    MxGemmArgs ge = g;
    asm volatile("s_waitcnt vmcnt(0)" : "+s"(ge.bias), "+s"(ge.gate), "+s"(ge.res), "+s"(ge.out0), "+s"(ge.out1) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    mx_epilogue(ge, acc, m0 + wm * 128 + fr, n0 + wn * 64, fq);
}

// ------------------------------------------------------------------------------------------------ quantise + down-project
constexpr int QB = 128;                    // rows per workgroup: 8 waves x 16
constexpr int QK = 128;                    // k per LDS chunk
constexpr int QP = QK * 2 + 16;            // LDS row pitch, bytes: 68 dwords, so 16 rows of a 16-byte read start 4 banks apart
constexpr int q_lds_bytes(int nj) { return (QB + nj * 16) * QP; }

template <int NJ>                          // R / 16 accumulators per wave
__global__ __launch_bounds__(512) void quant_rows_mx4_lr_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ codes,
                                                                 int64_t ldq, uint8_t* __restrict__ scales, int64_t lds,
                                                                 const bf16_t* __restrict__ Dn, int64_t ldd, bf16_t* __restrict__ T,
                                                                 int64_t ldt, int64_t M, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* xs = smem;
    char* ds = smem + QB * QP;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * QB;

    // loader: thread -> (row (tid >> 4) + 32 i, 16-byte chunk tid & 15); rows past M read row M - 1 and are never stored
    const int lr = tid >> 4, lc = tid & 15;
    const bf16_t* xp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = row0 + lr + 32 * i;
        xp[i] = x + (r < M ? r : M - 1) * ldx + lc * 8;
    }
    const bf16_t* dp = Dn + (int64_t)lr * ldd + lc * 8;
    const int st = lr * QP + lc * 16;
    u32x4 xr[4], dr[NJ / 2];
    auto load = [&](int kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xr[i] = *reinterpret_cast<const u32x4*>(xp[i] + kc * QK);
#pragma unroll
        for (int i = 0; i < NJ / 2; ++i) dr[i] = *reinterpret_cast<const u32x4*>(dp + 32 * i * ldd + kc * QK);
    };

    const int64_t row = row0 + wave * 16 + fr;
    const bool live = row < M;
    const int x_rd = (wave * 16 + fr) * QP + fq * 16;      // + kk * 64
    const int d_rd = fr * QP + fq * 16;                    // + nj * 16 * QP + kk * 64
    uint8_t* crow = codes + row * ldq + fq * 4;
    uint8_t* srow = scales + row * lds;
    f32x4 acc[NJ];
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) acc[nj] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunk = K / QK;
    load(0);
    for (int kc = 0; kc < nchunk; ++kc) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(xs + st + 32 * i * QP) = xr[i];
#pragma unroll
        for (int i = 0; i < NJ / 2; ++i) *reinterpret_cast<u32x4*>(ds + st + 32 * i * QP) = dr[i];
        __syncthreads();
        if (kc + 1 < nchunk) load(kc + 1);
#pragma unroll
        for (int kk = 0; kk < QK / 32; ++kk) {
            const u32x4 xa = *reinterpret_cast<const u32x4*>(xs + x_rd + kk * 64);
            float f[8];
            unpack8(xa, f);
            uint32_t amax = mx4_amax8(f);                  // the block = this lane's row over fq = 0 .. 3
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 16, 64));
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 32, 64));
            uint32_t e;
            const uint32_t w = mx4_codes8(f, amax, e);
            if (live) {
                *reinterpret_cast<uint32_t*>(crow + kc * (QK / 2) + kk * 16) = w;
                if (fq == 0) srow[kc * (QK / 32) + kk] = (uint8_t)e;
            }
#pragma unroll
            for (int nj = 0; nj < NJ; ++nj) {
                const u32x4 dn = *reinterpret_cast<const u32x4*>(ds + d_rd + nj * 16 * QP + kk * 64);
                acc[nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, dn), __builtin_bit_cast(bf16x8, xa), acc[nj], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // D = Dn . x^T: register r of accumulator nj is T[row fr][nj * 16 + 4 fq + r]
    if (live) {
#pragma unroll
        for (int nj = 0; nj < NJ; ++nj)
            *reinterpret_cast<u32x2*>(T + row * ldt + nj * 16 + fq * 4) = u32x2{pack_bf2(acc[nj][0], acc[nj][1]), pack_bf2(acc[nj][2], acc[nj][3])};
    }
}

// the rules for R and one of the bf16 rank operands [rows][cols] (T, Up, Dn)
bool lr_rank_ok(int R) { return R >= RC && R <= HV_MX_LR_MAX && R % RC == 0; }
bool lr_operand_ok(const void* p, int64_t ld, int64_t rows, int64_t cols) {
    return p && hv_aligned16(p) && !(ld & 7) && ld >= 0 && ld <= (1 << 22) && hv_pitch_ok(rows, ld, cols);
}

template <int RS>
int launch_gemm_lr(const LrGemmArgs& q, hipStream_t stream) {
    static HvPerDeviceOnce once;
    if (hv_set_max_lds(once, (const void*)gemm_mx4_lr_kernel<RS>, LDS_BYTES) != HV_OK) return HV_ERR_LAUNCH;
    gemm_mx4_lr_kernel<RS><<<dim3((unsigned)(q.g.tiles_m * q.g.tiles_n)), dim3(512), LDS_BYTES, stream>>>(q);
    return hv_check_launch();
}

template <int NJ>
int launch_quant_lr(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, const void* Dn, int64_t ldd, void* T,
                    int64_t ldt, int64_t M, int K, hipStream_t stream) {
    static HvPerDeviceOnce once;
    if (hv_set_max_lds(once, (const void*)quant_rows_mx4_lr_kernel<NJ>, q_lds_bytes(NJ)) != HV_OK) return HV_ERR_LAUNCH;
    quant_rows_mx4_lr_kernel<NJ><<<dim3((unsigned)((M + QB - 1) / QB)), dim3(512), q_lds_bytes(NJ), stream>>>(
        (const bf16_t*)x, ldx, (uint8_t*)codes, ldq, (uint8_t*)scales, lds, (const bf16_t*)Dn, ldd, (bf16_t*)T, ldt, M, K);
    return hv_check_launch();
}

}  // namespace

extern "C" int hv_quant_rows_mxfp4_lr(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, const void* Dn,
                                      int64_t ldd, void* T, int64_t ldt, int64_t M, int K, int R, hipStream_t stream) {
    if (!mx4_quant_args_ok(x, codes, scales, M, K, ldx, ldq, lds) || (K % QK) || !hv_aligned16(x) || !lr_rank_ok(R) ||
        !lr_operand_ok(Dn, ldd, R, K) || !lr_operand_ok(T, ldt, M, R))
        return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    switch (R / RC) {
        case 1: return launch_quant_lr<2>(x, ldx, codes, ldq, scales, lds, Dn, ldd, T, ldt, M, K, stream);
        case 2: return launch_quant_lr<4>(x, ldx, codes, ldq, scales, lds, Dn, ldd, T, ldt, M, K, stream);
        case 3: return launch_quant_lr<6>(x, ldx, codes, ldq, scales, lds, Dn, ldd, T, ldt, M, K, stream);
        default: return launch_quant_lr<8>(x, ldx, codes, ldq, scales, lds, Dn, ldd, T, ldt, M, K, stream);
    }
}

extern "C" int hv_gemm_mxfp4_lr(const void* A_codes, int64_t lda, const void* A_scales, int64_t ldas, const void* W_codes, int64_t ldw,
                                const void* W_scales, int64_t ldws, const void* bias, int M, int N, int K, void* out0, int64_t ld0, int act0,
                                int n_split, void* out1, int64_t ld1, int act1, const void* gate, const void* res, int64_t ld_res,
                                const void* T, int64_t ldt, const void* Up, int64_t ldu, int R, hipStream_t stream) {
    LrGemmArgs q{};
    if (K < HV_MX4_MIN_K || (K % KS) || !mx_gemm_args(q.g, A_codes, lda, A_scales, ldas, W_codes, ldw, W_scales, ldws, bias, M, N, K, out0, ld0,
                                                     act0, n_split, out1, ld1, act1, gate, res, ld_res))
        return HV_ERR_ARG;
    if (!lr_rank_ok(R) || !lr_operand_ok(T, ldt, M, R) || !lr_operand_ok(Up, ldu, N, R)) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    q.T = (const uint16_t*)T; q.Up = (const uint16_t*)Up; q.ldt = ldt; q.ldu = ldu;
    switch (R / RC) {
        case 1: return launch_gemm_lr<1>(q, stream);
        case 2: return launch_gemm_lr<2>(q, stream);
        case 3: return launch_gemm_lr<3>(q, stream);
        default: return launch_gemm_lr<4>(q, stream);
    }
}
