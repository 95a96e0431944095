// Stage B of the Motion-JPEG reader for frames without restart markers (include/hv_mjpeg_sync.h): a workgroup per restart interval, a
// lane per subsequence of its bytes, the self-synchronising decode of csrc/hv_mjpeg_sync.hpp (the text tools/mjpeg_sync_check.cpp runs
// on the host).
//
//   sync_kernel          256 lanes decode 256 consecutive subsequences side by side, lane 0 from the exact state, the others from a
//                        guess; lane j then takes lane j - 1's exit until no entry changes (rounds of 256 subsequences follow each
//                        other, each entered with the exact exit of the one before).  States are in LDS.  A workgroup prefix sum of
//                        the blocks each lane completed places the subsequences; every lane decodes once more from its exact entry
//                        and stores the non-zero coefficients into the zeroed blocks; three strip-wise prefix sums resolve the DC
//                        prediction.  A unit whose exact chain does not complete its blocks cleanly is decoded again by one lane
//                        with the serial decoder of stage B (hv_mjd_interval), which stores every block whole.
#include "hv_common.hpp"
#include "hv_mjpeg_sync.hpp"
#include "hv_wg_scan.hpp"
#include "../../include/hv_kernels.h"
#include "../../include/hv_mjpeg_read.h"
#include "../../include/hv_mjpeg_sync.h"

namespace {

constexpr int kLanes = HV_MJPEG_SYNC_LANES;
constexpr int kMaxWgs = 4096;
static_assert(kLanes == kWgScanThreads, "wg_scan_excl (csrc/hv_wg_scan.hpp) sums over the lanes");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

struct HuffBytes {
    uint8_t t[HV_MJPEG_HUFF_BYTES];
};

struct SyncArgs {
    const uint8_t* data;
    int64_t data_bytes;
    const int64_t *interval_begin, *interval_end;
    int Ri, ipf, sub;
    int64_t mpf, units;
    int16_t* coefs;
    int32_t *status, *iters;
    HuffBytes huff;
};

__global__ __launch_bounds__(kLanes) void sync_kernel(SyncArgs a) {
    __shared__ HvHuffTab s_tab[4];
    __shared__ HvSyncState s_exit[kLanes];
    __shared__ int s_scan[kLanes];
    __shared__ __attribute__((aligned(16))) int16_t s_stage[64];
    __shared__ uint8_t s_nat[64];
    const int tid = threadIdx.x;
    if (tid < 4) hv_mjd_build(a.huff.t + tid * kMjdTableBytes, &s_tab[tid]);
    if (tid < 64) s_nat[tid] = (uint8_t)hv_mjd_natural(tid);
    __syncthreads();
    for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int64_t t = u / a.ipf, k = u - t * a.ipf;
        const int64_t m0 = k * a.Ri;                                                   // Ri = 0: ipf = 1, k = 0
        const int64_t n = a.Ri == 0 || a.mpf - m0 < a.Ri ? a.mpf - m0 : a.Ri;
        const int64_t begin = clamp64(a.interval_begin[u], 0, a.data_bytes);
        const int64_t end = clamp64(a.interval_end[u], begin, a.data_bytes);
        const int expect = k < a.ipf - 1 ? 0xD0 + (int)(k & 7) : 0;
        const uint8_t* d = a.data + begin;
        const int64_t len = end - begin, n_blocks = n * 6;
        int16_t* out = a.coefs + (t * a.mpf + m0) * 384;

        for (int64_t i = tid; i < n * (HV_MJPEG_COEF_BYTES_PER_MCU / 16); i += kLanes) ((uint4*)out)[i] = uint4{0, 0, 0, 0};
        __syncthreads();

        const int64_t subs = (len + a.sub - 1) / a.sub, rounds = (subs + kLanes - 1) / kLanes;
        HvSyncState entry{0, 0, 0};
        int64_t total = 0;                                                             // blocks the exact chain has completed
        int its = 0;
        for (int64_t r = 0; r < rounds && entry.pos >= 0 && total < n_blocks; ++r) {
            const int64_t sub = r * kLanes + tid;
            const bool active = sub < subs;
            const int64_t sub_begin = active ? sub * a.sub : len;
            const int64_t sub_end = (len - sub_begin < a.sub ? len : sub_begin + a.sub) * 8;
            HvSyncState used{-2, 0, 0}, ex{-1, 0, 0};
            int32_t cnt = 0;
            for (int it = 0; it < kLanes + 1; ++it) {
                HvSyncState e = tid == 0 ? entry : it == 0 ? hv_mjs_guess(d, len, sub_begin) : s_exit[tid - 1];
                if (e.pos < 0) e = used;                                               // a dead exit says nothing: the entry in use stands
                const bool changed = active && !hv_mjs_same(e, used);
                __syncthreads();                                                       // every exit is read before one is replaced
                if (changed) {
                    used = e;
                    hv_mjs_lane<false>(d, len, s_tab, s_nat, e, sub_end, 0, 0, nullptr, &ex, &cnt);
                    s_exit[tid] = ex;
                }
                if (!__syncthreads_or(changed)) break;
                ++its;
            }
            // the lanes up to the first dead exit are exact, the ones behind it kept entries that mean nothing
            int dead_exits, round_blocks;
            const bool exact = wg_scan_excl(active && ex.pos < 0, s_scan, tid, dead_exits) == 0 && active;
            const int first = wg_scan_excl(exact ? cnt : 0, s_scan, tid, round_blocks);
            const int64_t in_round = subs - r * kLanes < kLanes ? subs - r * kLanes : kLanes;
            entry = dead_exits ? hv_mjs_dead() : s_exit[in_round - 1];
            if (exact) {
                int32_t again;
                hv_mjs_lane<true>(d, len, s_tab, s_nat, used, sub_end, total + first, n_blocks, out, &ex, &again);
            }
            total += round_blocks;
            __syncthreads();                                                           // the entry is read before the next round's exits
        }
        const bool clean = total >= n_blocks;
        __syncthreads();                                                               // every coefficient is stored
        if (clean) {
            for (int comp = 0; comp < 3; ++comp) {
                const int64_t count = comp == 0 ? n * 4 : n;
                int carry = 0;
                for (int64_t base = 0; base < count; base += kLanes) {
                    const int64_t i = base + tid;
                    int16_t* p = out + hv_mjs_dc_block(comp, i < count ? i : 0) * 64;
                    const int v = i < count ? *p : 0;
                    int strip;
                    const int before = wg_scan_excl(v, s_scan, tid, strip);
                    if (i < count) *p = (int16_t)(uint16_t)(carry + before + v);
                    carry = (int)(int16_t)(uint16_t)(carry + strip);
                }
            }
            if (tid == 0) {
                a.status[u] = HV_MJD_OK;
                if (a.iters) a.iters[u] = its;
            }
        } else if (tid == 0) {
            a.status[u] = hv_mjd_interval(a.data, begin, end, expect, s_tab, s_nat, n, s_stage, out);
            if (a.iters) a.iters[u] = -1;
        }
        __syncthreads();
    }
}

bool shape_ok(int T, int H, int W) { return T >= 1 && H >= 1 && W >= 1 && H <= HV_YUV_MAX_SIDE && W <= HV_YUV_MAX_SIDE; }
int64_t mcus_per_frame(int H, int W) { return (int64_t)((W + 15) / 16) * ((H + 15) / 16); }

}  // namespace

extern "C" int hv_mjpeg_decode_coefs_sync(const void* data, int64_t data_bytes, const int64_t* interval_begin, const int64_t* interval_end,
                                          int T, int H, int W, int Ri, int ipf, const uint8_t* huff_tables, int sub_bytes, void* coefs,
                                          int64_t coef_bytes, int32_t* status, int32_t* iters, hipStream_t stream) {
    if (!data || !interval_begin || !interval_end || !huff_tables || !coefs || !status) return HV_ERR_ARG;
    if (!shape_ok(T, H, W) || data_bytes < 0 || Ri < 0) return HV_ERR_ARG;
    if (sub_bytes < HV_MJPEG_SYNC_MIN_SUB || sub_bytes > HV_MJPEG_SYNC_MAX_SUB) return HV_ERR_ARG;
    const int64_t mpf = mcus_per_frame(H, W);
    if (ipf != (Ri == 0 ? 1 : (mpf + Ri - 1) / Ri) || (int64_t)T * ipf > 0x7fffffff) return HV_ERR_ARG;
    if (coef_bytes < hv_mjpeg_coef_bytes(T, H, W) || ((uintptr_t)coefs & 15) != 0) return HV_ERR_ARG;
    if ((((uintptr_t)interval_begin | (uintptr_t)interval_end) & 7) != 0 || (((uintptr_t)status | (uintptr_t)iters) & 3) != 0) return HV_ERR_ARG;
    if (!hv_mjd_tables_ok(huff_tables)) return HV_ERR_ARG;
    SyncArgs a{(const uint8_t*)data, data_bytes, interval_begin, interval_end, Ri, ipf, sub_bytes, mpf, (int64_t)T * ipf, (int16_t*)coefs, status,
               iters, {}};
    for (int i = 0; i < HV_MJPEG_HUFF_BYTES; ++i) a.huff.t[i] = huff_tables[i];
    sync_kernel<<<dim3((unsigned)(a.units < kMaxWgs ? a.units : kMaxWgs)), dim3(kLanes), 0, stream>>>(a);
    return hv_check_launch();
}
