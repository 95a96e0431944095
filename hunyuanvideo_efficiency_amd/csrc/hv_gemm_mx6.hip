// MXFP6 linears (opt-in; include/hv_gemm_mx6.h holds the format contract): the block-scaled e2m3 GEMM on
// v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 2: both operands FP6, 6 VGPRs each, E8M0 block scales applied inside the matrix
// pipe) and the two quantisers that produce its operands.
//
// GEMM main loop, one workgroup (8 waves, 2 along M x 4 along N) per 256 x 256 outputs, a wave 128 x 64 = 8 x 4 accumulators (the
// argument block, the deal of W rows to LDS rows and the epilogue are hv_mx_tile.hpp's, shared with hv_gemm_mx4.hip):
//   * a K-stage is 128 k = ONE matrix instruction per accumulator = 96 code bytes per row, 24 KiB per operand: three
//     global_load_lds_dwordx4 per thread and operand.  A lane's 32-k operand is bytes [24 fq, 24 fq + 24) of its row: 8-byte aligned
//     only, and 16-byte DMA chunk 1 (4) of a row is shared by k-blocks 0 and 1 (2 and 3).  The smallest piece the DMA can place freely
//     is therefore a row's k-HALF, 48 bytes = 3 chunks = the operands of two k-blocks.
//   * LDS layout of an operand: [k-half p][row][48 bytes], no padding (the DMA writes 1 KiB runs; chunk slot q = i * 512 + tid of its
//     i-th DMA holds chunk q % 3 of k-half q / 768 of row (q / 3) % 256).  A fragment is read as three 8-byte words at (p * 256 + row) *
//     48 + (fq & 1) * 24 + {0, 8, 16}.  Bank argument, for 64 banks of 4 bytes and 8-byte reads served 32 lanes at a time (lanes 0-31
//     = k-blocks 0, 1 = one k-half; lanes 32-63 the other): in units of 8 bytes the 16 rows of k-block 2p sit at 6 fr + j, those of
//     k-block 2p + 1 at 6 fr + 3 + j (j = which of the three words).  6 fr mod 32 runs over the 16 even residues, 6 fr + 3 over the 16
//     odd ones: the 32 lanes cover the 32 bank pairs exactly once, for every j, m-/n-repeat and wave (their bases are multiples of
//     768 = 3 * 256 bytes).  The 64-byte swizzle of hv_gemm_mx4.hip has no part in this; the row stride of 48 bytes does the work.
//   * scales: staged transposed exactly as in hv_gemm_mx4.hip (thread = row loads the stage's dword of four scale bytes, stores them
//     as bytes so that a lane's dword holds the scales of four 16-row groups for its k-block; op_sel picks the byte): three
//     ds_read_b32 per stage serve 32 matrix instructions.
//   * ring and registers.  3 slots x (2 x 24 + 2 x 1) KiB = 150 KiB of the CU's 160.  Beside the 128 accumulators, two waves per
//     SIMD leave room for 48 fragment registers (251 VGPRs, no scratch; with two sets of four A fragments, 72, the compiler spilled
//     19): ONE set of four W fragments (24) and two sets of TWO A fragments (an m-quarter each, 24) - both operands are
//     single-buffered across stages.  What that costs: a W fragment of stage t + 1 can only be read after the last instruction that
//     uses it in stage t, so those reads are threaded through the last m-quarter (n-repeat outermost: after the two instructions of
//     n-repeat ni, fragment ni of the next stage is read over it), and the last of them has only the first 6 instructions of the
//     next stage to land; an A quarter has the 8 instructions of the quarter before it.  The registers make up for the missing
//     fourth slot: when iteration t passes its barrier, all of stage t is in registers or consumed (W since iteration t - 1, the last
//     A quarter read before the third quarter's instructions), so its slot takes stage t + 3 at once and stages t + 2, t + 3 are in
//     flight while t + 1 is read.
//     Iteration t: [read A quarter q + 1 of t; 8 instructions on quarter q] for q = 0, 1, 2; counted vmcnt for the thread's own loads
//     of stage t + 1 (the 7 operations of t + 2 stay out), store its scale bytes, barrier; DMA + scale load of t + 3; read A
//     quarter 0 of t + 1; 8 instructions on quarter 3 with the W reads of t + 1 between them.  One barrier per stage.
// Both compiler hazards noted in hv_gemm.hip apply (same intrinsic): after the loop every accumulator is pinned under the full
// EXEC mask and the epilogue's pointers are made opaque, so neither a matrix instruction sinks into a masked region nor an epilogue
// load rises into the counted waits.
#include "hv_common.hpp"
#include "hv_ln_row.hpp"
#include "hv_mx_tile.hpp"
#include "hv_tile_order.hpp"
#include "../../include/hv_gemm_mx6.h"

namespace {

constexpr int BM = HV_MX6_BM, BN = HV_MX6_BN, KS = HV_MX6_KSTAGE, RING = HV_MX6_RING;
constexpr int ROW_BYTES = KS * 3 / 4;                // 96 code bytes per row and stage
constexpr int HALF_BYTES = ROW_BYTES / 2;            // a k-half: the operands of two k-blocks
constexpr int OP_BYTES = 256 * ROW_BYTES;            // one operand of one stage: 24 KiB
constexpr int SC_BYTES = 256 * (KS / 32);            // its scales: 1 KiB
constexpr int SLOT_BYTES = 2 * OP_BYTES + 2 * SC_BYTES;
constexpr int LDS_BYTES = RING * SLOT_BYTES;         // 150 KiB
constexpr int OPS_PER_STAGE = 7;                     // vector-memory operations a thread issues per stage: 6 DMA + 1 scale dword
constexpr int FRAG_STEP = 16 * HALF_BYTES;           // from one 16-row group to the next inside a k-half
static_assert(BM == 256 && BN == 256 && RING == 3 && LDS_BYTES <= 160 * 1024, "the loop below is written for this tile and ring");

typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(8))) int i32x8;
struct Frag6 { i32x2 lo, mid, hi; };                 // 24 bytes = the 32 codes of one (row, k-block), in memory order

__device__ __forceinline__ Frag6 read_frag(const char* p) {
    return Frag6{*reinterpret_cast<const i32x2*>(p), *reinterpret_cast<const i32x2*>(p + 8), *reinterpret_cast<const i32x2*>(p + 16)};
}

// one scaled FP6 matrix instruction: 6-register operands travel in the low registers of the builtin's 8-register type (cbsz = blgp =
// 2 makes the instruction read 6); OW / OA = byte of the scale register (op_sel), an immediate
template <int OW, int OA>
__device__ __forceinline__ f32x4 mfma_mx6(const Frag6& w, int sw, const Frag6& a, int sa, f32x4 c) {
    const i32x8 wv = {w.lo[0], w.lo[1], w.mid[0], w.mid[1], w.hi[0], w.hi[1], 0, 0};
    const i32x8 av = {a.lo[0], a.lo[1], a.mid[0], a.mid[1], a.hi[0], a.hi[1], 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv, av, c, 2, 2, OW, sw, OA, sa);
}

__global__ __launch_bounds__(512, 2) void gemm_mx6_kernel(MxGemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fq = lane >> 4;

    const TileMN tile = tile_of(xcd_linear_tile(), g.tiles_m, g.tiles_n);
    const int m0 = tile.tm * BM, n0 = tile.tn * BN;

    // ---- staging.  Codes: the i-th DMA of a thread fills chunk slot q = i * 512 + tid of the operand (see the header comment).  Tails
    // read clamped (valid) rows.
    uint32_t a_o[3], w_o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int q = i * 512 + tid, unit = q / 3;
        const int lr = unit & 255;
        const uint32_t chunk = (uint32_t)((unit >> 8) * HALF_BYTES + (q - unit * 3) * 16);
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
        char* dst = smem + (stage % RING) * SLOT_BYTES + wave * 1024;
        const char* as = opaque(a_tile + stage * ROW_BYTES);
        const char* ws = opaque(w_tile + stage * ROW_BYTES);
        const char* ss = opaque(sc_tile + stage * (KS / 32));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            uint32_t o = a_o[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(as + o), (lds_ptr_t)(dst + i * 8192), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            uint32_t o = w_o[i];
            asm volatile("" : "+v"(o));
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ws + o), (lds_ptr_t)(dst + OP_BYTES + i * 8192), 16, 0, 0);
        }
        uint32_t o = sc_o;
        asm volatile("" : "+v"(o));
        sreg = *(const __attribute__((address_space(1))) uint32_t*)(ss + o);      // (a global, not a flat, load: the asm hid the address space)
    };
    // (asm byte stores for the reason given in hv_gemm_mx4.hip: a compiler-visible LDS store would first drain every LDS-DMA in
    // flight.  The s_waitcnt lgkmcnt(0) before the stage's barrier covers them.)
    auto put_scales = [&](int stage, uint32_t sreg) {
        const uint32_t dst = (uint32_t)(uintptr_t)(lds_ptr_t)(smem + (stage % RING) * SLOT_BYTES + sc_dst);
        asm volatile("ds_write_b8 %0, %1\n\tds_write_b8 %0, %2 offset:64\n\tds_write_b8 %0, %3 offset:128\n\tds_write_b8 %0, %4 offset:192"
                     : : "v"(dst), "v"(sreg), "v"(sreg >> 8), "v"(sreg >> 16), "v"(sreg >> 24) : "memory");
    };

    // ---- fragments: lane (fr, fq) reads the 24 bytes of k-block fq of row (16-row group base + fr)
    const int frag_rd = (fq >> 1) * (256 * HALF_BYTES) + fr * HALF_BYTES + (fq & 1) * HV_MX6_BLOCK_BYTES;
    const int a_rd = wm * 128 * HALF_BYTES + frag_rd;                 // + mi * FRAG_STEP
    const int w_rd = OP_BYTES + wn * 64 * HALF_BYTES + frag_rd;       // + ni * FRAG_STEP
    const int sa_rd = 2 * OP_BYTES + (wm * 128 + lane) * 4;           // + h * 256
    const int sw_rd = 2 * OP_BYTES + SC_BYTES + (wn * 64 + lane) * 4;
    Frag6 aq[2][2], wf[4];
    int sa[2], sw[2];
    auto read_a = [&](auto Qc, int stage) {       // m-repeats 2 Q, 2 Q + 1 into buffer Q & 1; an even quarter brings its m-half's scales
        constexpr int Q = decltype(Qc)::value;
        const char* base = smem + (stage % RING) * SLOT_BYTES;
#pragma unroll
        for (int j = 0; j < 2; ++j) aq[Q & 1][j] = read_frag(base + a_rd + (2 * Q + j) * FRAG_STEP);
        if constexpr ((Q & 1) == 0) sa[Q >> 1] = *reinterpret_cast<const int*>(base + sa_rd + (Q >> 1) * 256);
    };

    f32x4 acc[8][4];
#pragma unroll
    for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    // 8 matrix instructions: m-quarter Q against the stage's four W fragments, n-repeat outermost.  NEXT: after the instructions of
    // n-repeat ni, W fragment ni of stage `next` is read over the one they used (the scales of that stage into the other sw).
    auto mma = [&](auto Pc, auto Qc, auto Nextc, int next) {
        constexpr int P = decltype(Pc)::value, Q = decltype(Qc)::value;
        constexpr bool NEXT = decltype(Nextc)::value != 0;
        const char* base = smem + (next % RING) * SLOT_BYTES;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        static_for(std::make_integer_sequence<int, 4>{}, [&](auto nic) {
            constexpr int ni = decltype(nic)::value;
            static_for(std::make_integer_sequence<int, 2>{}, [&](auto jc) {
                constexpr int j = decltype(jc)::value, mi = 2 * Q + j;
                acc[mi][ni] = mfma_mx6<ni, (mi & 3)>(wf[ni], sw[P], aq[Q & 1][j], sa[Q >> 1], acc[mi][ni]);
            });
            if constexpr (NEXT) {
                __builtin_amdgcn_sched_barrier(0);
                wf[ni] = read_frag(base + w_rd + ni * FRAG_STEP);
                if constexpr (ni == 3) sw[P ^ 1] = *reinterpret_cast<const int*>(base + sw_rd);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
    };

    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    const int nkt = g.K / KS;          // >= 4 (host side)
    // Register set (sw, sreg) of stage t: (t + par) & 1 with par = nkt & 1, so that the four tail iterations always see sets (0, 1, 0,
    // 1): an odd stage count is absorbed by ONE peeled iteration in front, not by a second copy of the tail.
    const int par = nkt & 1;
    uint32_t sreg[2], s0, s1, s2;
    // ---- prologue: stages 0, 1, 2 in flight and landed (one exposed latency per tile), the scales of stage 0 stored; the scale
    // dwords of stages 1 and 2 wait in the registers the first two iterations store from
    issue(0, s0);
    issue(1, s1);
    issue(2, s2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    put_scales(0, s0);
    sreg[0] = par ? s1 : s2;
    sreg[1] = par ? s2 : s1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) wf[ni] = read_frag(smem + w_rd + ni * FRAG_STEP);
    sw[0] = sw[1] = *reinterpret_cast<const int*>(smem + sw_rd);
    read_a(I0{}, 0);

    // R = min(nkt - t, 4), the stages left including this one, is a compile-time constant: the steady loop (R = 4) and the tail
    // iterations have no branches, and every vmcnt is a literal
    auto step = [&](auto Pc, auto Rc, int t) {
        constexpr int P = decltype(Pc)::value, R = decltype(Rc)::value;
        read_a(I1{}, t);
        mma(Pc, I0{}, I0{}, 0);
        read_a(I2{}, t);
        mma(Pc, I1{}, I0{}, 0);
        read_a(I3{}, t);
        mma(Pc, I2{}, I0{}, 0);
        if constexpr (R > 1) {
            // the thread's own loads of stage t + 1 are older than the OPS_PER_STAGE of stage t + 2 (if there is one)
            asm volatile("s_waitcnt vmcnt(%0)" : : "n"(R > 2 ? OPS_PER_STAGE : 0) : "memory");
            put_scales(t + 1, sreg[P ^ 1]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (R > 3) issue(t + 3, sreg[P ^ 1]);      // into the slot of stage t: every wave holds all it needs of it in registers
            read_a(I0{}, t + 1);
        }
        mma(Pc, I3{}, std::integral_constant<int, (R > 1)>{}, t + 1);
    };
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
    MxGemmArgs ge = g;
    asm volatile("s_waitcnt vmcnt(0)" : "+s"(ge.bias), "+s"(ge.gate), "+s"(ge.res), "+s"(ge.out0), "+s"(ge.out1) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    mx_epilogue(ge, acc, m0 + wm * 128 + fr, n0 + wn * 64, fq);
}

// ------------------------------------------------------------------------------------------------ quantisers
// Four adjacent lanes hold one block of 32 (8 elements each).  Everything after the block maximum is integer work, an exact fp32
// multiply by a power of two, and ONE fp32 addition whose rounding is the contract's: no other rounding happens here.
//   v < 1 (the subnormal codes, grid 1/8):  v + 2^20 is rounded by the adder to the ulp of 2^20 = 1/8, to nearest, ties to the even
//           multiple - the index is the sum's low mantissa bits;
//   v >= 1: the index is (exponent, top 3 mantissa bits) of v, rounded to nearest even on the bits below (a carry runs into the
//           exponent by itself), rebased so that 1.0 -> 8; 32 and above (v >= 7.75) saturate at 31.
__device__ __forceinline__ uint32_t e2m3_code(float x, float mul) {
    const float v = fabsf(x) * mul;
    const uint32_t u = __float_as_uint(v);
    const uint32_t lo = __float_as_uint(v + 1048576.0f) & 31u;
    const uint32_t hi = min(((u + 0x7FFFFu + ((u >> 20) & 1u)) >> 20) - (126u << 3), 31u);
    const uint32_t c = v < 1.0f ? lo : hi;
    return c ? c | ((__float_as_uint(x) >> 26) & 32u) : 0u;
}
// 8 values of a lane -> its 48 code bits; e = the block's E8M0 byte (the same in the block's four lanes; block maximum as mx4_quant8)
__device__ __forceinline__ uint64_t mx6_quant8(const float (&f)[8], uint32_t& e) {
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, __float_as_uint(f[j]) & 0x7FFFFFFFu);     // non-negative floats order as integers
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
    const uint32_t E = amax >> 23;
    e = E > 2 ? E - 2 : 0;
    const float mul = __uint_as_float((254u - e) << 23);         // 2^(127 - e): e <= 253, a normal number
    uint64_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= (uint64_t)e2m3_code(f[j], mul) << (6 * j);
    return w;
}
// The block's 192 bits are c0 | c1 << 48 | c2 << 96 | c3 << 144 (c_i = lane i's 48 bits): its three aligned 8-byte words are
// word i = c_i >> 16 i | c_(i+1) << (48 - 16 i), stored by lanes 0, 1, 2 of the block; lane 3 stores the scale byte.
__device__ __forceinline__ void mx6_store(uint64_t c, uint32_t e, int lane, uint8_t* block_codes, uint8_t* block_scale) {
    const uint64_t up = (uint64_t)(uint32_t)__shfl_down((int)(uint32_t)c, 1, 64) | ((uint64_t)(uint32_t)__shfl_down((int)(c >> 32), 1, 64) << 32);
    const int i = lane & 3;
    if (i < 3) *reinterpret_cast<uint64_t*>(block_codes + 8 * i) = (c >> (16 * i)) | (up << (48 - 16 * i));
    else *block_scale = (uint8_t)e;
}

__global__ __launch_bounds__(256) void quant_rows_mx6_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ codes,
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
        const uint64_t c = mx6_quant8(f, e);
        mx6_store(c, e, lane, codes + row * ldq + (ch >> 2) * HV_MX6_BLOCK_BYTES, scales + row * lds + (ch >> 2));
    }
}

// hv_ln_modulate_bf16 mode 0 up to the bf16 rounding (ln_mod_kernel's statistics and coefficients), then the quantiser
template <int MAXC>
__global__ __launch_bounds__(256) void ln_mod_mx6_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ add,
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
            const uint64_t w = mx6_quant8(v[c], e);
            mx6_store(w, e, lane, codes + row * ldq + (ch >> 2) * HV_MX6_BLOCK_BYTES, scales + row * lds + (ch >> 2));
        }
    }
}

bool quant_args_ok(const void* x, const void* codes, const void* scales, int64_t M, int K, int64_t ldx, int64_t ldq, int64_t lds) {
    if (!x || !codes || !scales || M < 0 || K <= 0 || (K % HV_MX6_BLOCK) || (ldx & 7) || (ldq & 7) || ((uintptr_t)codes & 7)) return false;
    return hv_pitch_ok(M, ldq, K / 4 * 3) && hv_pitch_ok(M, lds, K / HV_MX6_BLOCK) && hv_grid_x_ok((M + 3) / 4);
}

}  // namespace

extern "C" int hv_quant_rows_mxfp6(const void* x, int64_t ldx, void* codes, int64_t ldq, void* scales, int64_t lds, int64_t M, int K,
                                   hipStream_t stream) {
    if (!quant_args_ok(x, codes, scales, M, K, ldx, ldq, lds)) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    quant_rows_mx6_kernel<<<dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream>>>((const bf16_t*)x, ldx, (uint8_t*)codes, ldq,
                                                                                  (uint8_t*)scales, lds, M, K);
    return hv_check_launch();
}

extern "C" int hv_ln_modulate_mxfp6(const void* x, const void* shift, const void* scale, void* codes, int64_t ldq, void* scales,
                                    int64_t lds, int64_t M, int D, int64_t ldx, float eps, hipStream_t stream) {
    if (!quant_args_ok(x, codes, scales, M, D, ldx, ldq, lds) || D > 4096) return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    dim3 grid((unsigned)((M + 3) / 4)), block(256);
    ln_dispatch_maxc(D, [&](auto maxc) {
        ln_mod_mx6_kernel<decltype(maxc)::value><<<grid, block, 0, stream>>>((const bf16_t*)x, (const bf16_t*)shift, (const bf16_t*)scale,
                                                                             (uint8_t*)codes, ldq, (uint8_t*)scales, lds, M, D, ldx, eps);
    });
    return hv_check_launch();
}

extern "C" int hv_gemm_mxfp6(const void* A_codes, int64_t lda, const void* A_scales, int64_t ldas, const void* W_codes, int64_t ldw,
                             const void* W_scales, int64_t ldws, const void* bias, int M, int N, int K, void* out0, int64_t ld0, int act0,
                             int n_split, void* out1, int64_t ld1, int act1, const void* gate, const void* res, int64_t ld_res,
                             hipStream_t stream) {
    MxGemmArgs g{};
    if (K < HV_MX6_MIN_K || (K % KS) || !mx_gemm_args(g, A_codes, lda, A_scales, ldas, W_codes, ldw, W_scales, ldws, bias, M, N, K, out0, ld0, act0,
                                                     n_split, out1, ld1, act1, gate, res, ld_res))
        return HV_ERR_ARG;
    if (M == 0) return HV_OK;
    static HvPerDeviceOnce once;
    if (hv_set_max_lds(once, (const void*)gemm_mx6_kernel, LDS_BYTES) != HV_OK) return HV_ERR_LAUNCH;
    gemm_mx6_kernel<<<dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(512), LDS_BYTES, stream>>>(g);
    return hv_check_launch();
}
