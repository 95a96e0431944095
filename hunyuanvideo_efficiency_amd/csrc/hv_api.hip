#include "hv_common.hpp"
#include "../../include/hv_kernels.h"
extern "C" int hv_abi_version(void) { return 6; }   // 2: + hv_euler_step_f32_f32, hv_gemm_fp8 family; 3: conv gn_partial, sub-pixel upsampler conv; 4: hv_groupnorm_finalize_f16 takes partial_floats; 5: gn_partial entries (sum, centred sum of squares) + (0, count) per column pair; 6: + hv_video_metrics, hv_video_metrics_workspace_bytes
