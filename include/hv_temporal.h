/* Temporal interpolation: the entry point of csrc/hv_temporal.hip in libhv_kernels.so, under the conventions of include/hv_kernels.h (plain
 * pointers + sizes + a hipStream_t, caller-owned buffers, 0 = HV_OK, -1 = bad argument before anything is enqueued, -2 = launch failure).
 * It is declared here and not in hv_kernels.h: that header, its HV_ABI_VERSION and hv_temporal_resample_f16 (which keeps refusing every
 * mode but 0 | 1) stay as they are - this is a new symbol only - and this header has its own contract table (tests/temporal_contract.py,
 * checked without a GPU by tests/test_temporal_refusals_cpu.py).  The Python side parses this file as it parses hv_kernels.h
 * (hunyuanvideo_efficiency_amd/_abi.py: TEMPORAL_DECLS, TEMPORAL_MACROS); csrc/hv_temporal_torch_ops.cpp, generated from it by
 * tools/gen_torch_ops.py, registers torch.ops.hv.temporal_interp_f16. */
#ifndef HV_TEMPORAL_H
#define HV_TEMPORAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* The fork's t_ops interpolation with interp_mode "trilinear" on a channels-last activation x[T_in][HW][C] (fp16; pixel rows ldx elements
 * apart) -> out[T_in * s][HW][C] (rows ldo apart): F.interpolate(scale_factor=(s,1,1), mode="trilinear", align_corners=False)
 * (unet_causal_3d_blocks.py:853-911).  H and W have scale 1, so this is a linear interpolation along T alone.  Output frame t:
 *   num = max(2 t + 1 - s, 0), t0 = num / (2 s), t1 = min(t0 + 1, T_in - 1), lambda = (num mod 2 s) / (2 s) formed from the integers and
 *   rounded to fp32 once, y = (1 - lambda) x[t0] + lambda x[t1] in fp32, rounded to fp16 once.
 * Where lambda == 0 or t0 == t1 the output has the bits of x[t0] (NaN payloads and signed zeros included): s == 1 is the identity, and
 * the clamped leading and trailing frames are copies.  The result does not depend on how the launch is partitioned: two runs give the
 * same bits.
 * C % 8 == 0, ldx % 8 == 0, ldo % 8 == 0; T_in, HW, C > 0; s >= 1; T_in * s must fit an int and T_in * s * HW * C / 8 an int64;
 * ldo >= C when T_in * s * HW > 1 (output pitch rule); the input pitch is free; x and out not NULL and 16-byte aligned.  Violations are
 * HV_ERR_ARG.  out must not overlap x: the kernel assumes it and nothing checks it. */
int hv_temporal_interp_f16(const void* x, int64_t ldx, void* out, int64_t ldo, int T_in, int64_t HW, int C, int s, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HV_TEMPORAL_H */
