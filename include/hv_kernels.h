/* C ABI of libhv_kernels.so: the MI355X (gfx950) kernels behind the HunyuanVideo denoise / VAE-decode
 * hot path.  Plain pointers + sizes + a hipStream_t; no allocation inside, caller owns every buffer;
 * work is enqueued on `stream` and the call returns immediately.  Return: 0 = HV_OK, -1 = bad
 * argument (nothing launched), -2 = launch failure.  bf16 tensors are raw 16-bit words ("void*").
 *
 * The reference (c976237222/HunyuanVideo_efficiency) has no FFI of its own; its seams are Python call
 * sites.  Each entry point below names the reference arithmetic it replaces
 * (paths relative to /root/reference/hyvideo/).  The Python host side that mirrors the reference
 * interface (the modules/ directory of the hunyuanvideo_efficiency_amd package) binds these symbols with ctypes;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Argument contract (tests/abi_contract.py lists it row by row, tests/test_capi_refusals_cpu.py checks it without a GPU):
 *   - a bad argument is -1 (HV_ERR_ARG) BEFORE anything is enqueued; every condition an entry point enforces is stated in its comment.
 *     Common to all: a pointer not marked nullable must not be NULL; extents are positive unless an early-out is named; flags and
 *     enumerations take the listed values only; a shape whose launch grid or int index arithmetic would overflow (block counts
 *     above 2^31 - 1, grid.y / grid.z above 65535, element counts that do not fit the index type) is refused, never truncated.
 *   - early-outs return 0 (HV_OK) and touch no memory: M == 0, n == 0, n_rows == 0, n_q == 0, n_batch == 0, rows == 0 where named.
 *   - OUTPUT PITCH RULE, every entry point that stores rows: a row pitch of an OUTPUT below the width stored per row is HV_ERR_ARG when
 *     more than one row is stored (rows would overlap and two workgroups store to one address).  A single row is exempt: it has no
 *     neighbour, and hosts report arbitrary strides for extents of 1 (a [1, N] torch view may carry stride(0) < N).  INPUT pitches
 *     are not constrained beyond their alignment unless the comment says so (overlapping reads are well defined, pitch 0 broadcasts a
 *     row).  Documented aliasing stays legal: res may alias out0, hv_qknorm_rope_bf16 works in place.
 *   - the host queries (no stream argument) return 0 for every shape their kernel refuses and never a negative number.
 */
#ifndef HV_KERNELS_H
#define HV_KERNELS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* ABI version of this header (bumped on any signature change, or a change of what a caller-visible buffer holds);
 * tests/golden/abi_v<N>.json records the declarations of version N (python tools/gen_torch_ops.py --record-abi).
 *   2: + hv_euler_step_f32_f32, hv_gemm_fp8 family
 *   3: conv gn_partial, sub-pixel upsampler conv
 *   4: hv_groupnorm_finalize_f16 takes partial_floats
 *   5: gn_partial entries (sum, centred sum of squares) + (0, count) per column pair
 *   6: + hv_video_metrics, hv_video_metrics_workspace_bytes
 *   7: fp8 row scales floored at 2^-126 (finite codes for rows with 0 < amax < 448 * 2^-126), hv_vae_postprocess_f16_f32 keeps a NaN
 *   8: + hv_lpips_conv1_f32, hv_lpips_conv2d_f32, hv_lpips_maxpool_f32, hv_lpips_distance_f32, hv_lpips_distance_workspace_bytes
 *   9: + hv_temporal_spectrum, hv_temporal_spectrum_workspace_bytes
 *  10: + hv_i3d_preprocess, hv_i3d_conv3d_f32, hv_i3d_maxpool3d_f32, hv_i3d_head_f32
 *  11: + hv_yuv420_to_clip
 * The integer `#define HV_*` constants of this header are what a caller shares with the kernels (sizes, limits, table layouts);
 * the Python side reads them from here (hunyuanvideo_efficiency_amd/_abi.py). */
#define HV_ABI_VERSION 11
int hv_abi_version(void);       /* HV_ABI_VERSION of the header the library was compiled from */

/* K1: nn.LayerNorm(elementwise_affine=False, eps) followed by modulate()
 *     (modules/models.py:161-164,182-185,235,246,338; modules/modulate_layers.py:31-49; mlp_layers.py:115-117)
 * mode 0: out = LN(x) * bf16(1 + scale[d]) + shift[d]      (shift/scale may be NULL = absent)
 * mode 1: out = LN(x) * weight[d] + bias[d]                (token_refiner.py:33-35,56-58 affine LayerNorm)
 * x/out: [M, D] bf16 with row strides ldx/ldo (elements, % 8); D % 8 == 0, 0 < D <= 4096; M >= 0 (M == 0: HV_OK, nothing done), at most
 * 4 * (2^31 - 1) rows; ldo >= D when M > 1 (output pitch rule). */
int hv_ln_modulate_bf16(const void* x, const void* shift_or_bias, const void* scale_or_weight, void* out,
                        int64_t M, int D, int64_t ldx, int64_t ldo, float eps, int mode, hipStream_t stream);

/* K3+K4(+K5): per-head RMSNorm of q and k (modules/norm_layers.py:43,56-59) and apply_rotary_emb
 * (modules/posemb_layers.py:133-137,165-171) IN PLACE on fused QKV rows:
 *   row r: q head h at qkv[r*ld + h*128], k head h at qkv[r*ld + k_offset + h*128]  (v untouched).
 * Rows [0, n_rope) are rotated with cos/sin[r][128] (fp32); rows [n_rope, n_rows) are only normalised
 * (text tokens).  Writing in place into the joint [img|txt] QKV buffer removes the torch.cat of
 * models.py:195-197,358-359. head_dim must be 128; n_heads > 0; 0 <= n_rope <= n_rows <= 2^31 - 1 (n_rows == 0: HV_OK, nothing done);
 * cos_tab / sin_tab may be NULL when n_rope == 0; ld % 8 == 0, k_offset % 8 == 0.  The q and k heads must be different columns of the
 * row, k_offset >= n_heads * 128 (the row is rewritten in place: overlapping heads would be normalised twice), and the row must hold
 * them, ld >= k_offset + n_heads * 128, when n_rows > 1 (output pitch rule). */
int hv_qknorm_rope_bf16(void* qkv, const void* q_weight, const void* k_weight, const float* cos_tab,
                        const float* sin_tab, int64_t n_rows, int64_t n_rope, int n_heads, int head_dim,
                        int64_t ld, int64_t k_offset, float eps, hipStream_t stream);

/* The same, OUT OF PLACE with a scatter by head block (sequence parallelism, hyvideo/modules/attenion.py:169-180: the q / k chunk
 * that is normalised here is exchanged by an all-to-all over head groups next): head hv of row r (hv = 0 .. 2*n_heads-1 in the
 * q-then-k order of the source row) is stored at dst[(hv / heads_per_block) * dst_block_stride + r * dst_ld + (hv % heads_per_block)
 * * 128] - the [peer][row][heads of that peer] send layout - so no pack copy follows.  The source row is not modified: ld and k_offset
 * are only % 8 (q and k may be read from overlapping columns).  dst_ld % 8 == 0, dst_block_stride % 8 == 0, heads_per_block > 0;
 * dst_ld >= heads_per_block * 128 when n_rows > 1 (output pitch rule); the block stride is free (the layout [row][block][heads] has it
 * below a row). */
int hv_qknorm_rope_scatter_bf16(const void* qkv, const void* q_weight, const void* k_weight, const float* cos_tab,
                                const float* sin_tab, int64_t n_rows, int64_t n_rope, int n_heads, int head_dim, int64_t ld,
                                int64_t k_offset, float eps, void* dst, int64_t dst_ld, int heads_per_block,
                                int64_t dst_block_stride, hipStream_t stream);

/* K2/K7/K8/K10: nn.Linear on MFMA with fused epilogue.  C = A[M,K] . W[N,K]^T + bias
 *   (models.py:165,186,231,242,339-341,392-393; mlp_layers.py:53-59,117; embed_layers.py:40-59)
 * Columns [0, n_split) go to out0 (row stride ld0) with activation act0, columns [n_split, N) to
 * out1[., n - n_split] (row stride ld1) with act1 (act: 0 none, 1 GELU-tanh, 2 SiLU) - the single-stream
 * block's linear1 split + mlp_act (models.py:339-341,392).  n_split <= 0 or >= N: no split.
 * If gate != NULL: out = res + bf16(bf16(y) * gate[n])  (x + apply_gate(y, gate), models.py:231-250,393);
 * res may alias out0.  K % 64 == 0 (K >= 64), N % 8 == 0, all strides % 8 == 0 (ld1 and ld_res only where out1 / res are used); a split
 * needs out1 and n_split % 8 == 0; gate needs res; act0, act1 in 0..2; M >= 0 (M == 0: HV_OK, nothing done).  Output pitch rule, M > 1:
 * ld0 >= the columns of out0 (n_split, or N without a split), ld1 >= N - n_split.  ceil(M / 256) * ceil(N / 256) (N <= 128: / 128)
 * workgroups must fit 2^31 - 1. */
int hv_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, int M, int N, int K,
                 void* out0, int64_t ld0, int act0, int n_split, void* out1, int64_t ld1, int act1,
                 const void* gate, const void* res, int64_t ld_res, hipStream_t stream);

/* K9/K11: small-M Linear (M <= 4): out = act_out(W . act_in(x) + b).  act bit0: SiLU on input
 * (ModulateDiT / adaLN: Linear(SiLU(vec)), modulate_layers.py:27-28), bit1: SiLU on output
 * (MLPEmbedder / TimestepEmbedder hidden layer, mlp_layers.py:72-73, embed_layers.py:140-150).
 * addend (nullable, same layout as out): out = bf16(y) + addend, the bf16 `vec = vec + embedder(...)` adds of
 * models.py:621,631 and token_refiner.py:229.  1 <= M <= 4, N >= 1, K >= 8 and % 8, ldx % 8 == 0; act has no bits besides 0 and 1;
 * ldo >= N when M > 1 (output pitch rule; the [1, N] rows of the modulation vectors are exempt). */
int hv_linear_smallm_bf16(const void* x, const void* W, const void* bias, const void* addend, void* out, int M,
                          int N, int K, int64_t ldx, int64_t ldo, int act, hipStream_t stream);

/* timestep_embedding (modules/embed_layers.py:93-117,152-155): [cos(t f_i) | sin(t f_i)] in fp32 -> bf16;
 * t: n_t device floats, out [n_t, dim]; n_t > 0, dim > 0 and even, n_t * dim <= 2^31 - 1 (the kernel indexes with int). */
int hv_timestep_embedding_bf16(const float* t, void* out, int n_t, int dim, float max_period, hipStream_t stream);

/* K6/K6': softmax(scale * q k^T) v, bf16, head_dim 128, non-causal, over ONE contiguous key segment
 * (flash_attn_varlen_func / _flash_attn_forward of modules/attenion.py:107-120,181-207: the caller
 * issues one call per cu_seqlens segment).  q/k/v/o: token-major, head h at column h*128 of each row;
 * strides in elements (so q,k,v may point into one fused QKV buffer and o into a wider concat buffer).
 * workspace (nullable): caller-owned scratch, used in two steps:
 *   >= HV_ATTN_MIN_WORKSPACE_BYTES (256) and n_kv >= HV_ATTN_BOUND_MIN_KV (4096), n_heads <= 62: a pre-pass leaves max_k |k|^2 per head in its first 256
 *      bytes and the kernel bounds every score of a query row by |q'| |k|_max; a wave whose rows all have that bound within 90
 *      (log2 units) of their first tile's row max runs against it as a STATIC maximum (no row max per tile, never a rescale:
 *      +4 % at S = 119,056), any other wave keeps the online running maximum - same result up to the rounding of P;
 *   >= hv_attn_workspace_bytes(n_q, n_kv, n_heads) and a launch only a few workgroup rounds deep (e.g. 3 heads per rank under
 *      Ulysses-8): the key range is split in two halves processed by separate workgroups and merged (log-sum-exp) by a second
 *      tiny kernel: shorter makespan, same result up to fp32 rounding.
 * Without a workspace the single-pass kernel with the online maximum always runs.  A workspace must not be shared by launches
 * that can run concurrently (different streams).
 * head_dim must be 128; n_heads > 0; n_q >= 0 (n_q == 0: HV_OK, nothing done); 0 < n_kv <= 2^31 - 2049 when there are queries;
 * stride_q, stride_k, stride_v % 8 == 0, stride_o % 4 == 0; stride_o >= n_heads * 128 when n_q > 1 (output pitch rule);
 * ceil(n_q / 256) * n_heads workgroups must fit 2^31 - 1.  A workspace too small for a step only switches that step off. */
#define HV_ATTN_MIN_WORKSPACE_BYTES 256
#define HV_ATTN_BOUND_MIN_KV 4096
int hv_attn_fwd_bf16(const void* q, const void* k, const void* v, void* o, int64_t stride_q, int64_t stride_k,
                     int64_t stride_v, int64_t stride_o, int n_q, int n_kv, int n_heads, int head_dim,
                     float scale, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* bytes of scratch hv_attn_fwd_bf16 can use: the 256-byte bound area + the partials of a 2-way KV split (returned as int64);
 * 0 for extents hv_attn_fwd_bf16 refuses (n_q == 0 is its early-out: the bound area alone). */
int64_t hv_attn_workspace_bytes(int n_q, int n_kv, int n_heads);
/* crc32 of the generated steady-state iteration (csrc/hv_attention_w4_loop.inc, `#define HV_W4_LOOP_SIGNATURE`) the library's attention
 * kernel was compiled from: lets a host check that the library in front of it is the product build and not a timing experiment. */
int hv_attn_w4_loop_signature(void);        /* the 32 bits of the crc, as int */

/* Ring attention (hybrid Ulysses x Ring, xfuser `ring_degree > 1`: hyvideo/inference.py:171-175, call site
 * modules/attenion.py:169-180): the queries of one rank against ONE K/V chunk.  Leaves the unnormalised partial in slot(s)
 * [slot, slot+splits) of caller-owned buffers part_o = float[n_slots][n_q][n_heads][128], part_ml = float[n_slots][n_q][n_heads][2]
 * (running max in the log2 domain, denominator).  splits = 1 | 2: 2 halves the key range over two workgroup sets (load balance,
 * see hv_attn_suggest_splits) and fills two slots; it needs two key tiles (n_kv > 64).  Extents and input strides as hv_attn_fwd_bf16
 * (n_kv > 0 always); 0 <= slot, slot + splits <= n_slots.  n_q == 0: HV_OK, nothing done. */
int hv_attn_partial_bf16(const void* q, const void* k, const void* v, int64_t stride_q, int64_t stride_k, int64_t stride_v,
                         int n_q, int n_kv, int n_heads, int head_dim, float scale, void* part_o, void* part_ml,
                         int n_slots, int slot, int splits, hipStream_t stream);

/* Online-softmax merge of all n_slots partials: o = sum_s O_s 2^(m_s-m) / sum_s l_s 2^(m_s-m), written as bf16 rows.
 * n_heads > 0, n_slots > 0, n_q >= 0 (n_q == 0: HV_OK, nothing done), n_q * n_heads / 8 workgroups must fit 2^31 - 1; stride_o % 4 == 0
 * and >= n_heads * 128 when n_q > 1 (output pitch rule). */
int hv_attn_merge_bf16(const void* part_o, const void* part_ml, void* o, int64_t stride_o, int n_q, int n_heads, int n_slots,
                       hipStream_t stream);

/* 1 or 2: whether splitting the key range shortens the makespan of this launch shape on 256 CUs; 0 for extents hv_attn_fwd_bf16 refuses. */
int hv_attn_suggest_splits(int n_q, int n_kv, int n_heads);

/* K10 gather: fp32 latent [C,T,H,W] -> bf16 patch rows [T*(H/2)*(W/2), C*4] (embed_layers.py:40-59).  C, T > 0; H, W > 0 and even;
 * at most 256 * (2^31 - 1) (token, channel) pairs. */
int hv_patchify_f32_bf16(const float* x, void* A, int C, int T, int H, int W, hipStream_t stream);

/* unpatchify (models.py:697-710): y[tok][c*4+ph*2+pw] (row stride ldy, % 4) -> out[C,T,H,W] bf16.  C, T > 0; H, W > 0 and even;
 * at most 256 * (2^31 - 1) (token, channel) pairs. */
int hv_unpatchify_bf16(const void* y, void* out, int C, int T, int H, int W, int64_t ldy, hipStream_t stream);

/* K13: FlowMatchDiscreteScheduler.step (scheduling_flow_match_discrete.py:236-242):
 * sample_f32[i] += f32(model_out_bf16[i]) * dt.  0 <= n < 2^41 - 1024 (n == 0: HV_OK, nothing done). */
int hv_euler_step_f32(float* sample, const void* model_out_bf16, float dt, int64_t n, hipStream_t stream);

/* K13 with an fp32 velocity (the reference upcasts model_output, :239): sample_f32[i] += model_out_f32[i] * dt.  n as above. */
int hv_euler_step_f32_f32(float* sample, const float* model_out_f32, float dt, int64_t n, hipStream_t stream);

/* token_refiner.py:222-228: out[d] = sum_l x[l][d]*mask[l] / sum_l mask[l]  (mask NULL = plain mean).  L > 0, D > 0. */
int hv_masked_mean_bf16(const void* x, const int* mask, void* out, int L, int D, hipStream_t stream);

/* token_refiner.py:155-157: fully masked query rows see only key 0 -> their attention output is v[0].  D > 0, n_rows >= 0 (n_rows == 0:
 * HV_OK, nothing done), n_rows * D <= 256 * (2^31 - 1); ld >= D when n_rows > 1 (output pitch rule). */
int hv_broadcast_row_bf16(const void* src, void* dst, int64_t n_rows, int D, int64_t ld, hipStream_t stream);

/* C1 pack/unpack: batched strided 2-D copy dst[b][r][c] = src[b][r][c] with independent batch/row strides
 * (elements).  Re-lays tokens x heads for the Ulysses all-to-all (xfuser SeqAllToAll4D reached from
 * modules/attenion.py:169-180); the exchange itself is RCCL (torch.distributed "nccl"). cols % 8 == 0 (cols > 0), all four strides % 8;
 * 0 <= n_batch <= 65535 and 0 <= rows <= 2^31 - 1 (n_batch == 0 or rows == 0: HV_OK, nothing done); dst_ld >= cols when rows > 1 (output
 * pitch rule).  The batch strides are free: the unpack out[r][p * w + c] = recv[p][r][c] has dst_batch_stride = w below dst_ld. */
int hv_copy3d_bf16(const void* src, void* dst, int n_batch, int64_t rows, int cols, int64_t src_batch_stride,
                   int64_t src_ld, int64_t dst_batch_stride, int64_t dst_ld, hipStream_t stream);

/* K14: FP8 weight-only Linear (modules/fp8_optimization.py:50-53,55-80): out = bf16(bf16(w_e4m3fn[i]) * scale_bf16),
 * the per-forward dequantisation the reference performs before F.linear; the GEMM then runs on hv_gemm_bf16.
 * OCP e4m3fn (gfx950-native).  n > 0, n % 8 == 0. */
int hv_fp8_dequant_bf16(const void* w_e4m3fn, const void* scale_bf16, void* out_bf16, int64_t n, hipStream_t stream);

/* ---- FP8-MFMA path (opt-in; BASELINE.json configs[3] "fp8 weight path (CDNA4 fp8 MFMA)").  The reference's FP8 is weight-only
 * (fp8_optimization.py:50-80: e4m3fn weights + per-tensor `fp8_scale`, dequantised to bf16 every forward - that path is
 * hv_fp8_dequant_bf16 + hv_gemm_bf16).  Here the SAME stored weights feed v_mfma_scale_f32_16x16x128_f8f6f4 directly and the
 * activations are quantised per token: q = e4m3(clamp(x / s_row, +-448)), s_row = max(max|x_row| / 448, 2^-126) (1 for an all-zero
 * row), so
 *   y[m][n] = (sum_k qa[m][k] * qw[n][k]) * s_row[m] * fp8_scale + bias[n]   followed by hv_gemm_bf16's epilogues.
 * New error vs the reference path: the e4m3 rounding of the activations (2^-4 relative per element, averaging over K);
 * tolerance stated in tests/test_gpu_fp8_mfma.py.
 * The floor 2^-126 (the smallest normal fp32) keeps 1 / s_row finite: every code and scale is finite for finite input, also for a row
 * whose largest magnitude is below 448 * 2^-126 (a subnormal quotient would have a reciprocal of +inf and turn the row's zeros into
 * NaN codes); |x| / s_row <= 448 holds with the floor as without it.  Such a row quantises coarsely (it is < 2^-117 everywhere). */

/* K1 with an fp8 output: y = bf16(LN(x) * bf16(1 + scale) + shift) (hv_ln_modulate_bf16 mode 0), then per-row quantisation:
 * out_q [M, D] e4m3 bytes (row stride ldq bytes, % 16), out_row_scale [M] fp32.  D, M, ldx as hv_ln_modulate_bf16; ldq >= D when M > 1
 * (output pitch rule). */
int hv_ln_modulate_fp8(const void* x, const void* shift, const void* scale, void* out_q, float* out_row_scale, int64_t M,
                       int D, int64_t ldx, int64_t ldq, float eps, hipStream_t stream);

/* per-row quantisation of bf16 rows x[M, K] (row stride ldx elements) -> e4m3 rows + fp32 row scales (A operands that are not
 * LayerNorm outputs: attention output, GELU(MLP) hidden, the single block's [attn | mlp] concat).  K > 0 and % 8, ldx % 8 == 0,
 * ldq % 16 == 0; M >= 0 (M == 0: HV_OK, nothing done), at most 4 * (2^31 - 1) rows; ldq >= K when M > 1 (output pitch rule). */
int hv_quant_rows_fp8(const void* x, int64_t ldx, void* out_q, int64_t ldq, float* out_row_scale, int64_t M, int K,
                      hipStream_t stream);

/* C = (A_q . W_q^T) * a_row_scale[m] * w_scale + bias with hv_gemm_bf16's epilogue arguments.  A_q [M, K], W_q [N, K]: e4m3fn
 * bytes (row strides lda / ldw in bytes, % 16); w_scale_bf16: ONE bf16 on the device (the layer's `fp8_scale`).
 * K % 128 == 0, K >= 384; everything else as hv_gemm_bf16 (M == 0: HV_OK, nothing done). */
int hv_gemm_fp8(const void* A_q, int64_t lda, const float* a_row_scale, const void* W_q, int64_t ldw, const void* w_scale_bf16,
                const void* bias, int M, int N, int K, void* out0, int64_t ld0, int act0, int n_split, void* out1, int64_t ld1,
                int act1, const void* gate, const void* res, int64_t ld_res, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------------------
 * 3D causal VAE decode (hyvideo/vae).  Activations are fp16, CHANNELS-LAST: row = voxel (t*H + h)*W + w, C contiguous.
 * --------------------------------------------------------------------------------------------------------- */

/* fp16 Linear on MFMA (diffusers Attention to_q/to_k/to_v/to_out of the VAE mid block, unet_causal_3d_blocks.py:579-593;
 * 1x1x1 convs: post_quant_conv autoencoder_kl_causal_3d.py:115 and conv_shortcut unet_causal_3d_blocks.py:339-347).
 * out = A.W^T + bias; out_is_f32 (0 | 1): fp32 result (attention scores; no res then); res (nullable): out = res + f16(y).
 * K, N, strides, M == 0 and the workgroup limit as hv_gemm_bf16; ldo (in elements of the result type) >= N when M > 1 (output pitch rule). */
int hv_gemm_f16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, int M, int N, int K,
                void* out, int64_t ldo, int out_is_f32, const void* res, int64_t ld_res, hipStream_t stream);

/* K15 (+K17): CausalConv3d 3x3x3 = replicate-pad(W 1,1; H 1,1; T 2,0) + Conv3d (unet_causal_3d_blocks.py:49-75) as an
 * implicit GEMM; with up_t/up_hw the nearest upsample of UpsampleCausal3D.forward (:154-172: first frame x(1,2,2), others
 * x(2,2,2)) that precedes its conv is folded into the gather.  x: source [sT,sH,sW,Cin] (row stride ldx);
 * w_taps: [Cout][27][Cin] fp16 (tap = (dt*3 + dh)*3 + dw); out: [T*H*W, Cout]; res (nullable): out = res + f16(y)
 * (ResnetBlockCausal3D residual :413-415).  Cin % 64 == 0, Cout % 8 == 0 (callers zero-pad 16->64 and 3->8).
 * The source is addressed with 32-bit byte offsets: sT*sH*sW*ldx*2 must be < 4 GiB (HV_ERR_ARG otherwise).
 * T, H, W > 0 with T*H*W <= 2^31 - 1; up_t, up_hw 0 | 1 (up_t: T odd; up_hw: H, W even); ldx, ldo, ld_res % 8 == 0; ldo >= Cout when
 * T*H*W > 1 (output pitch rule).
 * gn_partial (nullable, device fp32 [hv_gn_partial_rows(T*H*W)][Cout][2], gn_partial_floats = its size): the epilogue also
 * leaves the GroupNorm statistics of the tensor it stores - per 64-row block b and pair of adjacent columns (c, c+1), c even, over the
 * k valid values: gn_partial[b][c] = (S = sum, C2 = sum of (x - S/k)^2), gn_partial[b][c+1] = (0, k); every entry written once, in a
 * fixed order - so the GroupNorm that follows (ResnetBlockCausal3D.norm1/norm2 :395-411, conv_norm_out) needs no pass over the
 * activation: hv_groupnorm_finalize_f16 folds them.  HV_ERR_ARG if the buffer is too small. */
int hv_conv3d_causal_f16(const void* x, int64_t ldx, const void* w_taps, const void* bias, void* out, int64_t ldo,
                         int T, int H, int W, int Cin, int Cout, int up_t, int up_hw, const void* res,
                         int64_t ld_res, float* gn_partial, int64_t gn_partial_floats, hipStream_t stream);

/* rows of the gn_partial buffer for an output of M rows: one per 64 output rows, whole 256-row tiles; 0 unless 0 < M <= 2^31 - 1. */
int64_t hv_gn_partial_rows(int64_t M);
/* ... and for hv_conv3d_upsampled_subpixel_f16, whose M tiles are formed per parity class (some blocks cover no row: zeros); 0 for a
 * source grid that kernel refuses. */
int64_t hv_subpixel_gn_partial_rows(int sT, int sH, int sW, int up_t);

/* UpsampleCausal3D (unet_causal_3d_blocks.py:154-172: nearest x2 in H, W - and in T with the first frame kept single - then the
 * causal 3x3x3 conv) in its SUB-PIXEL form.  The outputs of one parity class (t, h, w mod 2) read every source voxel through a
 * fixed subset of the 27 taps, so each class is a conv over the SOURCE grid with 2 pre-summed taps per upsampled axis:
 *     H/W, even output 2k:   w0 x[k-1] + (w1+w2) x[k]        odd output 2k+1: (w0+w1) x[k] + w2 x[k+1]      (indices clamped = replicate pad)
 *     T,   even frame  2k:   w0 x[k-1] + (w1+w2) x[k]        odd frame 2k-1:  (w0+w1) x[k-1] + w2 x[k]      (k-1 clamped at 0 = causal pad)
 * 8 taps (12 when only H, W are upsampled) instead of 27: 3.4x (2.25x) fewer flops than hv_conv3d_causal_f16 with up_t/up_hw, and
 * algebraically the same function.  x: source [sT,sH,sW,Cin]; out: [T2, 2 sH, 2 sW, Cout], T2 = 2 sT - 1 (up_t) or sT;
 * w_sub: [classes][Cout][ntap*Cin] fp16, class = pt*4 + ph*2 + pw (8, up_t) or ph*2 + pw (4); tap_table: device int32
 * [classes][ntap], source offset of each tap as (ot+8) | (oh+8)<<4 | (ow+8)<<8.  Weights and table come from the caller
 * (vae_ops.subpixel_weights): a summed weight is rounded to fp16 once ("fast": <= 2 fp16 ulp from the 27-tap form), or its rounding
 * residue rides along as an extra tap with the same offset ("exact": products exact, as in the 27-tap form).
 * Cin a power of two >= 256, Cout > 128 and % 8 == 0 (the decoder's 256- and 512-channel upsamplers).  1 <= ntap <= 27, up_t 0 | 1,
 * 0 < sT <= 254, 0 < sH, sW <= 4096 (packed gather coordinates), output voxels <= 2^31 - 1, source below 4 GiB as above; ldx, ldo % 8 == 0,
 * ldo >= Cout (output pitch rule).
 * gn_partial: as for hv_conv3d_causal_f16, [hv_subpixel_gn_partial_rows(sT, sH, sW, up_t)][Cout][2]. */
int hv_conv3d_upsampled_subpixel_f16(const void* x, int64_t ldx, const void* w_sub, const void* tap_table, int ntap,
                                     const void* bias, void* out, int64_t ldo, int sT, int sH, int sW, int Cin, int Cout,
                                     int up_t, float* gn_partial, int64_t gn_partial_floats, hipStream_t stream);

/* DecoderCausal3D tail (vae.py:283-294: conv_norm_out -> SiLU -> conv_out): GroupNorm apply + SiLU + the 3x3x3 causal conv to
 * Cout <= 3 channels in two streaming passes instead of an HBM pass and an implicit GEMM that stages every activation nine times:
 *   planes[tap][voxel][c] = sum_ch w[c][ch][tap] * act(x[voxel][ch] * affine[ch][0] + affine[ch][1])      fp32, every voxel read once
 *   out[voxel][c] = fp16(bias[c] + sum_{tap = 0..26} planes[tap][clamped tap-shifted voxel][c])           padding rule of hv_conv3d_causal_f16
 * x: channels-last fp16 [T*H*W][ldx >= Cin]; affine (nullable: x is used as it is): fp32 [Cin][2] (scale, shift) as
 * hv_groupnorm_finalize_f16 / hv_groupnorm_affine_f16 leave it, applied in fp32 and rounded to fp16 once - the arithmetic of
 * hv_groupnorm_apply_f16; silu: 0 | 1.  w_frag: the weights in MFMA fragment order, fp16 [7][4][64][8]: row block nb, k step ks, lane l,
 * element j = w[c][ks*32 + 8*(l>>4) + j][tap] with 4*tap + c = 16*nb + (l & 15), zero for c == 3, tap >= 27 and channels >= Cin
 * (vae_ops.cout4_weight_fragments builds it).  out: [T*H*W][ldo]: ldo >= 8: columns Cout..7 are written as zeros (one 16-byte store).
 * planes: workspace of hv_conv3d_cout4_planes_floats(T*H*W) floats (HV_ERR_ARG if planes_floats is below it; the query returns 0 unless
 * 0 < M <= 256 * (2^31 - 1), the most voxels the kernel takes).  Cin % 32 == 0, 0 < Cin <= 128, 0 < Cout <= 3; ldx % 8 == 0; ldo >= Cout
 * and % 8 from 8 on; x, out, w_frag 16-byte aligned; bias is required.  The sum over the taps is
 * taken in a fixed order: results are run-to-run identical (not bit-identical to hv_conv3d_causal_f16: another summation order). */
int hv_conv3d_cout4_f16(const void* x, int64_t ldx, const float* affine, int silu, const void* w_frag, const void* bias, void* out,
                        int64_t ldo, int T, int H, int W, int Cin, int Cout, float* planes, int64_t planes_floats, hipStream_t stream);
int64_t hv_conv3d_cout4_planes_floats(int64_t M);

/* DownsampleCausal3D (VAE encoder, unet_causal_3d_blocks.py:185-247): the same padding as hv_conv3d_causal_f16, then the 3x3x3
 * conv with stride 1|2 per axis (the fork's t_ops `downsample_stride` override, :737-742, changes these strides).
 * x: source [sT,sH,sW,Cin]; out: [T*H*W, Cout] with T = (sT-1)/stride_t + 1, H = (sH-1)/stride_h + 1, W likewise.  Cin, Cout, ldx, ldo,
 * the 4 GiB source rule and the output pitch rule as hv_conv3d_causal_f16; sT*sH*sW <= 2^31 - 1. */
int hv_conv3d_causal_strided_f16(const void* x, int64_t ldx, const void* w_taps, const void* bias, void* out, int64_t ldo,
                                 int sT, int sH, int sW, int Cin, int Cout, int stride_t, int stride_h, int stride_w,
                                 hipStream_t stream);

/* The fork's temporal ops on a channels-last activation x[T_in][HW][C] (unet_causal_3d_blocks.py:657-672,764-783,884-907).
 * mode 0: F.pad(replicate, k-1 frames in front) + F.avg_pool3d((k,1,1), stride (s,1,1)) -> T_out = (T_in-1)/s + 1;
 * mode 1: F.interpolate(scale_factor=(s,1,1), mode="nearest") -> T_out = T_in*s (must fit an int).  C % 8 == 0, ldx, ldo % 8 == 0,
 * T_in, HW > 0, s >= 1, k >= 1 in mode 0, mode 0 | 1; T_out * HW * C / 8 must fit an int64; ldo >= C when T_out * HW > 1 (output pitch rule). */
int hv_temporal_resample_f16(const void* x, int64_t ldx, void* out, int64_t ldo, int T_in, int64_t HW, int C, int mode,
                             int k, int s, hipStream_t stream);

/* K16 pass 1+2: GroupNorm statistics (nn.GroupNorm(32, C, eps 1e-6, affine), unet_causal_3d_blocks.py:302,323) folded
 * into a per-channel affine: affine_out[2c] = rstd_g*w[c], affine_out[2c+1] = b[c] - mean_g*rstd_g*w[c].  The moments are summed
 * about a pivot per group (its first channel in row 0), so an offset group mean does not cancel the variance.
 * partial_ws: caller workspace of partial_ws_floats floats (>= 2*C; 2*C*1024 for full parallelism).  M > 0; C % 8 == 0, 8 <= C <= 2048,
 * C / 8 a divisor of 256; groups a power of two <= 64 dividing C; ldx % 8 == 0. */
int hv_groupnorm_affine_f16(const void* x, int64_t ldx, int64_t M, int C, int groups, float eps, const void* weight,
                            const void* bias, float* partial_ws, int64_t partial_ws_floats, float* affine_out,
                            hipStream_t stream);

/* K16 pass 2 alone: the same affine from statistics a conv epilogue already took (hv_conv3d_causal_f16 `gn_partial`):
 * partial [nrow][C][2] fp32 followed by HV_GN_FOLD_WS_FLOATS floats of fold workspace IN THE SAME BUFFER (the fp64 fold scratch
 * starts at the next even float index behind the partials), M = rows of the activation they cover.  partial_floats = size of that
 * buffer in floats: HV_ERR_ARG unless it is >= align2(nrow*C*2) + HV_GN_FOLD_WS_FLOATS (a buffer sized for the conv alone is too
 * small and is refused, never overrun).  Folded in fp64 in a fixed order: sum x^2 of an entry = C2 + S^2 / k, so the variance
 * var = Q/n - mean^2 cancels only in fp64.  The epilogue credits each pair of adjacent channels to the even one, so C / groups must
 * be even (HV_ERR_ARG otherwise).  nrow, M > 0; C and groups as hv_groupnorm_affine_f16 (any C % 8 == 0). */
#define HV_GN_FOLD_WS_FLOATS 16384
int hv_groupnorm_finalize_f16(const float* partial, int64_t partial_floats, int64_t nrow, int64_t M, int C, int groups, float eps,
                              const void* weight, const void* bias, float* affine_out, hipStream_t stream);

/* K16 pass 3: y = [SiLU](x*affine[2c] + affine[2c+1]) -> fp16 (norm + nonlinearity, unet_causal_3d_blocks.py:361-363,399-405).
 * silu 0 | 1; M > 0; C % 8 == 0, 8 <= C <= 2048; ldx, ldy % 8 == 0; ldy >= C when M > 1 (output pitch rule). */
int hv_groupnorm_apply_f16(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t M, int C, const float* affine,
                           int silu, hipStream_t stream);

/* K18: P = softmax(scale * S) row-wise, fp32 -> fp16, columns [valid, cols_pad) zero-filled (K padding of the P.V GEMM).
 * causal_block = 0: valid = cols for every row.  causal_block = HW > 0: the frame-causal mask of prepare_causal_attention_mask
 * (unet_causal_3d_blocks.py:38-46) - row r belongs to frame r / HW and sees the keys of frames <= its own: valid =
 * min(cols, (r / HW + 1) * HW) - so one launch covers all frames of a tile.  rows, cols > 0, cols_pad >= cols, causal_block >= 0;
 * ld_p >= cols_pad when rows > 1 (output pitch rule). */
int hv_softmax_rows_f32_f16(const float* S, int64_t ld_s, void* P, int64_t ld_p, int rows, int cols, int cols_pad,
                            float scale, int causal_block, hipStream_t stream);

/* [R][C] -> [C][R] for 16-bit elements (V^T for the P.V GEMM).  R, C > 0, R <= 65535 * 32; ld_dst >= R when C > 1 (output pitch rule). */
int hv_transpose_16b(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int R, int C, hipStream_t stream);

/* latent crop: fp32 z[C,T,H,W] region (element strides) -> channels-last fp16 [T,H,W,Cpad] (zero-padded channels):
 * the tile slicing of autoencoder_kl_causal_3d.py:443,520 + the fp16 cast of autocast.  C, T, H, W > 0, Cpad >= C, T*H*W*Cpad must fit
 * an int64; the source strides are free. */
int hv_vae_latent_tile_f16(const float* z, int64_t sc, int64_t st, int64_t sh, int64_t sw, int C, int T, int H, int W,
                           int Cpad, void* out, hipStream_t stream);

/* K19: blend_v / blend_h / blend_t (autoencoder_kl_causal_3d.py:344-360) on strided [C,T,H,W] fp16 views:
 * b[i] = f16(f16(a[i]*(1 - y/extent)) + f16(b[i]*(y/extent))), y = index along `axis` (0..3); dims[axis] <= extent, extent > 0.
 * a_strides, b_strides (int64 [4]) and dims (int [4], all > 0, product within an int64) are HOST arrays, read before the call returns. */
int hv_vae_blend_f16(const void* a, const int64_t* a_strides, void* b, const int64_t* b_strides, const int* dims,
                     int axis, int extent, hipStream_t stream);

/* crop + concat of tiles (autoencoder_kl_causal_3d.py:463-465,531-537): strided 4-D copy of 16-bit elements; host arrays as above. */
int hv_copy4d_16b(const void* src, const int64_t* src_strides, void* dst, const int64_t* dst_strides, const int* dims,
                  hipStream_t stream);

/* K20 tail: (image / 2 + 0.5).clamp(0, 1) in fp16 then .float() (pipeline_hunyuan_video.py:1090-1092).  A NaN input gives a NaN, as
 * torch's clamp keeps it (it is not clamped to 0).  n > 0. */
int hv_vae_postprocess_f16_f32(const void* x, float* out, int64_t n, hipStream_t stream);

/* Reconstruction scoring (evaluation/compute_metrics.py:31-41 compute_psnr / compute_ssim of the fork, without the mp4 round trip):
 * per-frame statistics of two videos a, b [C,T,H,W] (C = 1 | 3; dtype 0 = fp16, 1 = fp32; element strides *_sc, *_st, *_sh, W contiguous)
 * on the 8-bit frames save_videos_grid would write: q = (uint8) trunc(clamp(rescale ? (x + 1) / 2 : x, 0, 1) * 255), every step in fp32
 * as utils/file_utils.py:frames_uint8 rounds it.  Outputs, one row per frame: sse int64 [T] = sum (qa - qb)^2 over C,H,W;
 * minmax int32 [T][4] = min(qa), max(qa), min(qb), max(qb); ssim_sum fp64 [T][C] = sum over the (H-6) x (W-6) window positions of the
 * SSIM map of channel c (7x7 uniform window, sample covariance, K1 0.01, K2 0.03, data range max(qa) - min(qa) of the frame:
 * skimage.metrics.structural_similarity's defaults as the fork calls it); 0 for a frame whose `a` is constant (the caller's rule gives
 * such a frame SSIM 1).  Box moments are exact integers; the map value is fp32, summed in fp64 in a fixed order (no atomics: run-to-run
 * identical).  passes: 3 = both; 1 = the statistics pass alone (sse, minmax); 2 = the SSIM pass alone, reading the data range from a
 * `minmax` an earlier statistics pass filled (how tools/bench_metrics.py times the two separately).  workspace: >= hv_video_metrics_workspace_bytes(C, T, H, W) bytes, 16-byte aligned.  H < 7 or W < 7, T > 65535 and
 * negative or overlapping strides (*_sh < W) are HV_ERR_ARG (the workspace query returns 0 for the shapes among them), as are H or W above
 * 65536, C other than 1 | 3, T < 1, dtype or rescale other than 0 | 1, passes outside 1..3 and a workspace that is too small. */
int hv_video_metrics(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st,
                     int64_t b_sh, int dtype, int C, int T, int H, int W, int rescale, int passes, void* sse, void* minmax,
                     void* ssim_sum, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t hv_video_metrics_workspace_bytes(int C, int T, int H, int W);

/* LPIPS, AlexNet trunk (the fork's evaluation/compute_metrics.py:43-62,116,142-146 calling lpips.LPIPS(net="alex"):
 * rebuttal/common_metrics_on_video_quality/lpips/lpips.py:112-144,147-167, lpips/__init__.py:13-15, lpips/pretrained_networks.py:56-94),
 * one entry point per kernel; every step is fp32 as in the reference, the convolutions run on the fp32-input MFMA (each output element
 * one k-ordered fmaf chain).  Features are channels-last fp32 [image][h][w][C]; the 2T images of a call are the T frames of the first
 * video followed by the T frames of the second.  Conv weights are k-major [Kpad][Cout] (Kpad = K rounded up to 32, zero rows behind K),
 * 16-byte aligned.
 *
 * First layer (pretrained_networks.py:66-67,78-80 slice1 = Conv2d(3, 64, 11, 4, 2) + ReLU on the ScalingLayer's output, lpips.py:118,
 * 147-154, and the input scaling of compute_metrics.py:44-60): reads the two videos a, b [3,T,H,W] as hv_video_metrics does (dtype,
 * element strides, rescale, the same 8-bit quantiser) and feeds the conv lut[c][q], a host-built float [3][256] holding
 * ((float32(q / 255.0) * 2 - 1) - shift[c]) / scale[c]; padding is zero in that scaled domain.  k = (c * 11 + ky) * 11 + kx, K = 363
 * (w is [384][64]).  y: [2T][(H - 7) / 4 + 1][(W - 7) / 4 + 1][64].  H or W < 31 (the smallest input with a tap-5 pixel) is HV_ERR_ARG, as
 * are H or W above 65536, T outside [1, 32767], dtype or rescale other than 0 | 1, negative strides and *_sh < W. */
int hv_lpips_conv1_f32(const void* a, int64_t a_sc, int64_t a_st, int64_t a_sh, const void* b, int64_t b_sc, int64_t b_st,
                       int64_t b_sh, int dtype, int T, int H, int W, int rescale, const float* lut, const float* w,
                       const float* bias, float* y, hipStream_t stream);

/* Layers 2-5 (pretrained_networks.py:68-77,82-90: Conv2d(64, 192, 5, padding=2), Conv2d(192, 384, 3, padding=1), Conv2d(384, 256, 3,
 * padding=1), Conv2d(256, 256, 3, padding=1), each + ReLU): y[N][OH][OW][Cout] = relu(conv(x[N][H][W][Cin], stride 1, zero padding
 * `pad`) + bias), OH = H + 2 pad - ksize + 1.  k = (ky * ksize + kx) * Cin + ci.  Cin % 32 == 0, Cout % 64 == 0, 0 <= pad < ksize <= 11
 * (ksize >= 1); Cin in [32, 4096], Cout in [64, 4096]; N >= 1, H, W in [1, 65536], OH, OW >= 1, N*H*W and N*OH*OW <= 2^31 - 1; x (and w)
 * 16-byte aligned. */
int hv_lpips_conv2d_f32(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Cout,
                        int ksize, int pad, hipStream_t stream);

/* MaxPool2d(kernel_size=3, stride=2) between taps 1-2 and 2-3 (torchvision alexnet features[2], [5]; pretrained_networks.py:66-71):
 * x [N][H][W][C] -> y [N][(H - 3) / 2 + 1][(W - 3) / 2 + 1][C], C % 4 == 0, 4 <= C <= 4096, H, W in [3, 65536], N >= 1, x and y 16-byte
 * aligned, output elements / 4 <= 256 * (2^31 - 1). */
int hv_lpips_maxpool_f32(const float* x, float* y, int N, int H, int W, int C, hipStream_t stream);

/* One tap's distance (lpips.py:122-130 with lpips/__init__.py:13-15 normalize_tensor and the NetLinLayer 1x1 conv of lpips.py:157-167):
 * f [2T][P][C] (P pixels), lin [C]; out[t * 5 + layer] = sum over pixels of sum_c lin[c] (f0 / (sqrt(sum f0^2) + 1e-10) - f1 / (...))^2
 * in fp64, frame t comparing image t with image T + t (the caller divides by P: spatial_average, and adds the five taps).  C <= 384.
 * Workgroup partials go to `workspace` (>= hv_lpips_distance_workspace_bytes(T, P) bytes, 8-byte aligned) and are folded in a fixed
 * order: no atomics, run-to-run identical, and a frame's bits do not depend on T.  T in [1, 65535], P >= 1, C >= 1, layer in 0..4
 * (the query returns 0 for T, P outside these). */
int hv_lpips_distance_f32(const float* f, const float* lin, int T, int64_t P, int C, int layer, double* out, void* workspace,
                          int64_t workspace_bytes, hipStream_t stream);
int64_t hv_lpips_distance_workspace_bytes(int T, int64_t P);

/* Temporal spectra (the fork's theory_analysis.ipynb cells 2, 4, 5: np.abs(np.fft.fft(signal, axis=0)).mean(axis=1) over the pixel time
 * series of the 8-bit gray frames of a clip, and over every (channel, h, w) series of latent_dist.mean): per-bin SUMS over all series of
 * one x [C,T,H,W] (dtype 0 = fp16, 1 = fp32; element strides sc, st, sh, W contiguous, as hv_video_metrics) of |X_k| and |X_k|^2,
 * k = 0 .. T/2 (K = T/2 + 1 bins; the caller divides by the series count and mirrors bin T - k from bin k).
 * mode 0 (gray8, C = 3): one series per pixel; R, G, B are quantised to the byte save_videos_grid would write (the quantiser of
 * hv_video_metrics) and combined to the integer luma (wr R + wg G + wb B + round) >> shift, which must stay a byte: weights and round
 * >= 0, shift <= 22, (wr + wg + wb) * 255 + round < 256 << shift.  mode 1 (raw, any C): one series per (c, h, w), the value cast to fp32.
 * Arithmetic: bin 0 is sum_t x_t itself (mode 0: exact integers, also in pow_sum while a partial sum stays below 2^53; mode 1: an fp32
 * chain in frame order, its square rounded to fp32).  Bins k >= 1 transform d_t = x_t - x_0 (exact in mode 0, one fp32 rounding in
 * mode 1; the DFT of the constant x_0 vanishes there): re_k, im_k = sum_t d_t * twiddle, each one fp32 fmaf chain on the fp32-input MFMA;
 * |X_k|^2 = fl(fl(re^2) + fl(im^2)), |X_k| = sqrtf of it; both summed over series in fp64 through workgroup partials folded in a fixed
 * order (no atomics: run-to-run identical).
 * twiddle: host-built fp32 [Tpad][64 * ncol], Tpad = T rounded up to HV_SPECTRUM_BK (32), ncol = max(1, ceil((T/2) / HV_SPECTRUM_BINS)),
 * 16-byte aligned, twiddle_floats >= Tpad * 64 * ncol: column 64 j + c holds cos (c < 32) or sin (c >= 32) of 2 pi ((k t) mod T) / T for
 * bin k = 1 + 32 j + (c & 31) (HV_SPECTRUM_BINS = 32 bins per column tile), zero for k > T/2 and in rows t >= T.
 * workspace: >= hv_temporal_spectrum_workspace_bytes(mode, C, T, H, W) bytes, 8-byte aligned.  T < 1, T > HV_SPECTRUM_MAX_T, C != 3 in
 * mode 0, H or W outside [1, 65536], negative or overlapping strides (sh < W) are HV_ERR_ARG (the workspace query returns 0 for the
 * shapes among them), as are C outside [1, 65536], H * W above 2^31 - 1, mode, dtype or rescale other than 0 | 1, a weight above 2^22 and
 * buffers that are too small. */
#define HV_SPECTRUM_MAX_T 1024
#define HV_SPECTRUM_BK 32
#define HV_SPECTRUM_BINS 32
int hv_temporal_spectrum(const void* x, int64_t sc, int64_t st, int64_t sh, int dtype, int mode, int C, int T, int H, int W,
                         int rescale, int wr, int wg, int wb, int round, int shift, const float* twiddle, int64_t twiddle_floats,
                         double* mag_sum, double* pow_sum, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int64_t hv_temporal_spectrum_workspace_bytes(int mode, int C, int T, int H, int W);

/* Frechet Video Distance, I3D logits (the fork's rebuttal/common_metrics_on_video_quality/calculate_fvd.py:28-48 with method='videogpt':
 * fvd/videogpt/fvd.py:21-65 preprocessing, fvd/videogpt/pytorch_i3d.py the Inception-I3D network), one entry point per kernel, every step
 * fp32 as in the reference.  Features are channels-last fp32 [voxel = (t * H + h) * W + w][C] with a row pitch (ldx, ldy, in elements): the
 * pointer may address a column slice of a wider buffer, so the four branches of an Inception module (pytorch_i3d.py:127-132) write straight
 * into their slice of the module's output and the torch.cat of :132 never happens.  Element offsets are 64-bit.
 *
 * Preprocessing (fvd.py:21-60 preprocess / preprocess_single): x [3,T,H,W] read as hv_video_metrics reads a video (dtype 0 = fp16, 1 =
 * fp32, element strides, W contiguous, `rescale`, the same 8-bit quantiser: the reference's (videos * 255).astype(uint8) on [0, 1] frames
 * is that truncation), then b / 255 in fp32, bilinear resize to RH x RW (F.interpolate(mode='bilinear', align_corners=False): source
 * coordinate max(0, fmaf((float)in / (float)out, dst + 0.5, -0.5)), written as one fma), centre crop of 224 x 224 at ((RH - 224) / 2,
 * (RW - 224) / 2), (v - 0.5) * 2.  y: [T][224][224][4] fp32, channel 3 = 0 (the first conv reads 4-channel voxels), 16-byte aligned.  RH, RW
 * come from the caller (fvd.py:32-36: the shorter side 224, the other ceil(side * (224 / min(H, W))) in the host's double arithmetic);
 * HV_ERR_ARG unless the shorter side's is 224 and the other's >= 224 (H == W: either side, since that double arithmetic gives 225 x 224 for
 * some sizes, e.g. 200 x 200).  The 8-bit frames never reach memory.  T, H, W in [1, 65536], RH, RW <= 2^20, dtype and rescale 0 | 1,
 * x_sh >= W, no negative stride. */
int hv_i3d_preprocess(const void* x, int64_t x_sc, int64_t x_st, int64_t x_sh, int dtype, int T, int H, int W, int RH, int RW, int rescale,
                      float* y, hipStream_t stream);

/* Unit3D (pytorch_i3d.py:78-103: F.pad with zeros, Conv3d, eval-mode BatchNorm3d or bias, ReLU or none) as an implicit GEMM on the
 * fp32-input MFMA (each output element one k-ordered fmaf chain):  y[o][n] = act(sc[n] * sum_k x[window of o][k] w[k][n] + sh[n]),
 * act = ReLU if relu else identity; sc, sh: the BatchNorm folded by the caller (sc = gamma / sqrt(var + eps), sh = beta - mean * sc), or
 * sc = 1, sh = bias for the logits layer.  x: [T*H*W][ldx >= Cin]; y: [OT*OH*OW][ldy >= Cout], O = ceil(extent / stride) per axis (the
 * "same" rule of :81-83).  Kernel extents 1 | 3 | 7 and strides 1 | 2 per axis; pad_*: cells of zero padding in FRONT of each axis (< the
 * kernel extent; the caller applies compute_pad :71-75 and :88-93), cells behind the input read as zero too.  w: k-major [Kpad][Cout],
 * k = ((dt * kh + dh) * kw + dw) * Cin + ci, Kpad = K rounded up to 32 with zero rows, 16-byte aligned.  Cin % 4 == 0 and Cout % 4 == 0,
 * both in [4, 4096] (the first layer reads the 4-channel output of hv_i3d_preprocess); ldx % 4 == 0, x 16-byte aligned.  T, H, W in
 * [1, 65536] with T*H*W <= 2^31 - 1; relu 0 | 1; ldy >= Cout also for a single output voxel. */
int hv_i3d_conv3d_f32(const float* x, int64_t ldx, const float* w, const float* sc, const float* sh, float* y, int64_t ldy, int T, int H,
                      int W, int Cin, int Cout, int kt, int kh, int kw, int stride_t, int stride_h, int stride_w, int pad_t, int pad_h,
                      int pad_w, int relu, hipStream_t stream);

/* MaxPool3dSamePadding (pytorch_i3d.py:7-34: F.pad with zeros, then MaxPool3d): kernel extents 1..3, strides 1 | 2 per axis, pad_* cells in
 * front (< the kernel extent), output extents ceil(extent / stride).  A window cell outside the input holds 0 AND TAKES PART in the
 * maximum: a border window over all-negative inputs gives 0.  A NaN cell makes its windows NaN, as
 * torch's max_pool3d does.  C % 4 == 0, 4 <= C <= 4096; ldx, ldy % 4 == 0 and >= C; x, y 16-byte aligned; T, H, W as hv_i3d_conv3d_f32. */
int hv_i3d_maxpool3d_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int T, int H, int W, int C, int kt, int kh, int kw,
                         int stride_t, int stride_h, int stride_w, int pad_t, int pad_h, int pad_w, hipStream_t stream);

/* The tail of InceptionI3d.forward (pytorch_i3d.py:276-285,310-315): AvgPool3d([2,7,7], stride 1) on x [T][7][7][1024] (row pitch ldx),
 * the 1024 -> 400 logits layer with bias (w k-major [1024][400]), the mean over the T - 1 time positions: out [400].  fp32 in a fixed
 * order: a pooled value is the sum of its 98 cells in memory order / 98, a logit one k-ordered fmaf chain, the mean summed in time order.
 * workspace: >= (T - 1) * 1024 floats, 16-byte aligned.  HV_ERR_ARG unless H == W == 7, C == 1024 and 2 <= T <= HV_I3D_HEAD_MAX_T;
 * ldx >= C and % 4, x 16-byte aligned. */
#define HV_I3D_HEAD_MAX_T 4096
int hv_i3d_head_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* out, int T, int H, int W, int C,
                    float* workspace, int64_t workspace_floats, hipStream_t stream);

/* Raw planar YUV 4:2:0 frames -> clip tensor (the fork's dataset_processor/yuv_tensor.py: the frame loop :108-140 with
 * cv2.cvtColor(COLOR_YUV2BGR_I420 / _YV12 / _NV12) :128-133, the target size :207-212 and cv2.resize :167, COLOR_BGR2RGB :237, ToTensor
 * :238, the [3,T,H,W] stack :249 and 2x - 1 :250) in one pass; the 8-bit RGB frames never reach memory.  Integer arithmetic and table lookups
 * only.  UNPINNED RESTATEMENT: cv2 is not part of this environment, so the bytes below are OpenCV's rule as far as it can be
 * established without executing it (tests/test_yuv_cpu.py anchors them independently).
 * raw: device bytes of the first frame; T frames at a pitch of W * H * 3 / 2 bytes: the Y plane [H][W], then by `layout`
 *   HV_YUV_I420: U [H/2][W/2], V [H/2][W/2];   HV_YUV_YV12: V, U;   HV_YUV_NV12: [H/2][W/2] interleaved (U, V) pairs.
 * Pixel (y, x) takes the chroma sample (y >> 1, x >> 1), no chroma interpolation.  Colour, BT.601 limited range, int32, `>>` arithmetic:
 *   yy = max(0, Y - 16) * 1220542;   R = clamp((yy + 1673527 (V - 128) + 2^19) >> 20, 0, 255);
 *   G = clamp((yy - 852492 (V - 128) - 409993 (U - 128) + 2^19) >> 20, 0, 255);   B = clamp((yy + 2116026 (U - 128) + 2^19) >> 20, 0, 255).
 * OH == H and OW == W: no resize (ytab, xtab unused, may be NULL).  Otherwise a 2-tap bilinear filter per axis on the 8-bit R, G, B - this
 * project's own rule, modelled on cv2.resize(INTER_LINEAR) but not claimed equal to its bytes - from the caller's tables: ytab int32
 * [OH][2], xtab int32 [OW][2], entry d = (first source index s, weight c1 of the second index min(s + 1, extent - 1)), c1 in
 * [0, 2^HV_YUV_COEF_BITS], c0 = 2^HV_YUV_COEF_BITS - c1 (dataset.resize_tables builds them; the kernel clamps an entry into range):
 *   h_r = c0x P[y_r][x0] + c1x P[y_r][x1] for the two source rows,   q = (c0y h_0 + c1y h_1 + 2^21) >> 22.
 * out: element (c, t, y, x) of channel order R, G, B at out[c * sc + t * st + y * sh + x] (element strides, W contiguous, as
 * hv_video_metrics reads a video), dtype 0 = fp16, 1 = fp32, holding vtab[q]: the caller's 256 entries in the output dtype
 * (dataset.yuv_value_table: the bits of (float(q) / 255) * 2 - 1, for fp16 rounded once more).  All frame and output offsets are 64-bit.
 * HV_ERR_ARG, nothing launched: odd or non-positive W or H, a side (W, H, OH, OW) above HV_YUV_MAX_SIDE, T < 1, OH or OW < 1, out or vtab
 * not aligned to the output dtype, differing sizes without
 * both tables, an unknown layout or dtype, negative strides or strides under which two cells of the output share an address. */
#define HV_YUV_I420 0
#define HV_YUV_YV12 1
#define HV_YUV_NV12 2
#define HV_YUV_COEF_BITS 11
#define HV_YUV_MAX_SIDE 16384
int hv_yuv420_to_clip(const void* raw, int T, int layout, int W, int H, void* out, int dtype, int64_t sc, int64_t st, int64_t sh,
                      int OH, int OW, const int* ytab, const int* xtab, const void* vtab, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HV_KERNELS_H */
