#include "hv_common.hpp"
#include "../../include/hv_kernels.h"
extern "C" int hv_abi_version(void) { return 7; }   // 2: + hv_euler_step_f32_f32, hv_gemm_fp8 family; 3: conv gn_partial, sub-pixel upsampler conv; 4: hv_groupnorm_finalize_f16 takes partial_floats; 5: gn_partial entries (sum, centred sum of squares) + (0, count) per column pair; 6: + hv_video_metrics, hv_video_metrics_workspace_bytes; 7: fp8 row scales floored at 2^-126 (finite codes for rows with 0 < amax < 448 * 2^-126), hv_vae_postprocess_f16_f32 keeps a NaN
