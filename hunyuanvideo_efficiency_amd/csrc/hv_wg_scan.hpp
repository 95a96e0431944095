// The workgroup prefix sum of the Motion-JPEG readers (csrc/hv_mjpeg_read.hip, csrc/hv_mjpeg_sync.hip): one copy.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kWgScanThreads = 256;

// exclusive prefix sum of v over a workgroup of kWgScanThreads threads; total = the sum.  s: kWgScanThreads ints of LDS, free again on
// return.
__device__ inline int wg_scan_excl(int v, int* s, int tid, int& total) {
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < kWgScanThreads; off <<= 1) {
        const int a = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    total = s[kWgScanThreads - 1];
    const int ex = s[tid] - v;
    __syncthreads();
    return ex;
}
