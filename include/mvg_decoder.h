/*
 * mvg_decoder.h -- C ABI of libmvgformer_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary of the MVGFormer decoder hot path.  Plain pointers and sizes,
 * no torch / ATen types.  All pointers are DEVICE pointers unless marked "host".
 * Every entry point enqueues work on `stream` (a hipStream_t passed as void*;
 * NULL = the default stream), never synchronises, never allocates, never
 * mutates its inputs, and returns 0 (hipSuccess) or a hipError_t / MVG_E_* code.
 * No exception crosses this boundary.
 *
 * Reference interfaces replaced (paths relative to the MVGFormer reference tree):
 *   - pybind module `Deformable` : lib/models/ops/src/vision.cpp:24-27
 *       deform_forward  : lib/models/ops/src/deform.h:32-50  -> deform_cuda_forward,
 *                         lib/models/ops/src/cuda/deform_cuda.cu:31-91,
 *                         kernel lib/models/ops/src/cuda/deform_im2col_cuda.cuh:248-309
 *       deform_backward : lib/models/ops/src/deform.h:53-72  -> deform_cuda_backward,
 *                         lib/models/ops/src/cuda/deform_cuda.cu:94-164, kernels cuh:312-930
 *   - the ATen op chains of ProjAttn.forward (lib/models/ops/modules/projattn.py:115-204),
 *     DQDecoderLayer.forward (lib/models/dq_decoder.py:850-1045) and the DLT
 *     triangulation (lib/mvn/utils/multiview.py:170-269) -> the mvg_* stage entry points.
 *
 * Layout conventions (see DESIGN.md "Data layout in HBM"):
 *   image index n = v*B + b (view-major, like dq_decoder.py:560);  Lq = NQ*J joint tokens;
 *   value / feat : (N_img, S, C) channels-last, level l at rows [start_l, start_l+H_l*W_l);
 *   dtype code   : MVG_F32 = 0, MVG_BF16 = 1 (bf16 storage, fp32 accumulation).
 */
#ifndef MVG_DECODER_H
#define MVG_DECODER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVG_F32 0
#define MVG_BF16 1

#define MVG_E_BADARG 10001   /* shape / alignment / dtype not supported            */
#define MVG_E_NOGPU 10002    /* no gfx950 device visible                            */

/* floats per packed camera record, one record per image n = v*B + b            */
#define MVG_CAM_STRIDE 48
/* record layout (float index):
 *   0..8  R (row-major 3x3)       9..11 T (camera centre, mm)   12 fx 13 fy 14 cx 15 cy
 *   16..18 k1 k2 k3               19,20 p1 p2
 *   21..26 crop affine 2x3 (orig px -> network px; lib/utils/transforms.py:72-112)
 *   27..32 inverse crop affine 2x3 (meta['inv_affine_trans'][:2])
 *   33,34 wh = 2*center (orig image size)   35 clamp_max (max of wh over the batch)
 *   36,37 network image size (w,h)          38..47 reserved (0)
 */

/* Library / device identification.  Returns 0 and fills arch (e.g. "gfx950") if a
 * usable device is present; MVG_E_NOGPU otherwise.  Host-only. */
int mvg_device_info(char* arch_out, int arch_len, int* cu_count);
const char* mvg_version(void);
/* Kernel-variant knobs for A/B measurements.  PROCESS-GLOBAL and not thread-safe: a value set here applies to every later call
 * of every entry point from every thread, whatever the stream or device; set knobs before the first launch (or from one thread
 * while nothing is in flight), never as per-request state.  Host-only.  Env MVG_TUNE="key=value,..." sets them at load time.
 *   "gsamp_threads" = 128 | 256 | 512 | 1024, "gsamp_map" = 0 | n : workgroup size and XCD block mapping of the G-sampling kernel
 *       (chunks of n slot blocks per XCD, 0 = one head per XCD);  "gsamp_pipe" = 0 | 1 | 2 : its gather loop double-buffered from 32 768 pairs per launch on / always / never;
 *       "gsamp_lds_pad" / "chain_a_lds_pad" = bytes (probes): unused dynamic LDS per sampler / chain-A workgroup, caps the workgroups per
 *       CU (occupancy sweeps: tools/r06_sampler_probe.py, tools/r06_fusion_emul.py);
 *   "gfused_chunk" = 0 | n : the same mapping for the fp32 G-sampling kernel;  "fwd_map" = 0 | 1 | 2 : decomposition of mvg_msda_forward;
 *   "auto_small" = 1 | 0 : launches with few rows (a rank's shard of a query-sharded run) use smaller workgroups / tiles in the
 *       sampler, chain A (64-row tiles up to 320 tiles of 128 rows) and chain B (32-row tiles up to 128 tiles of 64 rows);
 *   "chain_rm" = 64 | 128 | 256 : rows per tile of mvg_chain_attn_pose;  "f32h_rows" = 0 | 32 | 64 : rows per tile of the fp32 chains;
 *   "wreg_grid" = n : persistent workgroups of mvg_pyramid_group_ws;  "bin_multi" = 1 | 0 : multi-workgroup binning for large Lq;
 *   "linear_tiles" = 0 | 1 | 2 : tile shapes of mvg_linear*;
 *   "f32_split" = 1 | 0 : fp32 GEMMs of mvg_linear* as six bf16 MFMA products on operands split into three bf16 parts (default) or
 *       as v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain); with 0 the Python layer also stands the fused fp32 kernels down.
 * Every knob but f32_split, auto_small (chain B's 32-row tiles sum the FFN in another order) and chain_rm = 256 selects
 * bit-identical results (tests/test_hip_parity.py: test_every_kernel_variant_behind_a_tuning_knob). */
int mvg_set_tuning(const char* key, int value);
/* Getter and enumerator of the same knobs (process-global and not thread-safe like the setter; host-only): for 0 <= index < the
 * number of knobs stores the knob's key (a static string) and its current value and returns 0, MVG_E_BADARG otherwise. */
int mvg_tuning_knob(int index, const char** key, int* value);

/* ---- Deformable.deform_forward / deform_backward (deform.h:32-72) -------------------
 * value (N,S,M,D); spatial_shapes (L,2) int64 (H,W); level_start_index (L,) int64;
 * sampling_loc (N,Lq,M,L,P,2) (x,y) in [0,1]; attn_weight (N,Lq,M,L,P); out (N,Lq,M*D).
 * f32: every tensor float32 (AT_DISPATCH_FLOATING_TYPES' float case, deform_cuda.cu:75).
 * bf16: value/out bf16, sampling_loc/attn_weight float32, fp32 accumulation. */
int mvg_msda_forward_f32(const float* value, const int64_t* spatial_shapes,
                         const int64_t* level_start_index, const float* sampling_loc,
                         const float* attn_weight, float* out,
                         int N, int S, int M, int D, int L, int Lq, int P, void* stream);
int mvg_msda_forward_bf16(const void* value, const int64_t* spatial_shapes,
                          const int64_t* level_start_index, const float* sampling_loc,
                          const float* attn_weight, void* out,
                          int N, int S, int M, int D, int L, int Lq, int P, void* stream);
/* f64: every tensor float64 -- the `double` case of AT_DISPATCH_FLOATING_TYPES (deform_cuda.cu:75,145), for gradcheck-style
 * calls; plain one-thread-per-output-channel kernels, no fast path.  mvg_msda_backward_f64: grad_value must be zero-filled
 * by the caller like the f32 form; grad_sampling_loc / grad_attn_weight are zeroed and accumulated by the entry point. */
int mvg_msda_forward_f64(const double* value, const int64_t* spatial_shapes,
                         const int64_t* level_start_index, const double* sampling_loc,
                         const double* attn_weight, double* out,
                         int N, int S, int M, int D, int L, int Lq, int P, void* stream);
int mvg_msda_backward_f64(const double* value, const int64_t* spatial_shapes,
                          const int64_t* level_start_index, const double* sampling_loc,
                          const double* attn_weight, const double* grad_output,
                          double* grad_value, double* grad_sampling_loc, double* grad_attn_weight,
                          int N, int S, int M, int D, int L, int Lq, int P, void* stream);
/* grad_value (N,S,M,D) must be zero-filled by the caller (at::zeros_like, deform_cuda.cu:132);
 * grad_sampling_loc / grad_attn_weight are fully overwritten.  Deterministic for a fixed
 * launch geometry only up to the atomic-add order in grad_value (as the reference, cuh:135-162). */
int mvg_msda_backward_f32(const float* value, const int64_t* spatial_shapes,
                          const int64_t* level_start_index, const float* sampling_loc,
                          const float* attn_weight, const float* grad_output,
                          float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                          int N, int S, int M, int D, int L, int Lq, int P, void* stream);

/* Deterministic, atomics-free-in-fp32 form of mvg_msda_backward_f32 for D = 32 (csrc/msda_bwd.hip): the samples are binned
 * by destination tile, a workgroup per tile gathers its value patch into LDS and accumulates grad_value there as 64-bit
 * fixed-point integers (integer addition is associative: no dependence on the order of arrival), grad_sampling_loc /
 * grad_attn_weight are reduced over the 32 channels with a fixed shuffle tree.  Bit-reproducible run to run; every output is
 * fully overwritten (grad_value need not be zero-filled).  workspace: device scratch of
 * mvg_msda_backward_det_workspace(...) bytes (0 = shape not supported: D != 32, L*P > 256, Lq >= 2^24 -- use the
 * atomic form).  shapes_host / starts_host: HOST int64 arrays (the level table is a kernel argument here).
 * Non-finite entries of grad_output are not propagated into grad_value (the fixed-point scale is the largest finite |g|). */
size_t mvg_msda_backward_det_workspace(int N, int S, int M, int D, int L, int Lq, int P, const int64_t* shapes_host);
int mvg_msda_backward_det_f32(const float* value, const int64_t* shapes_host, const int64_t* starts_host,
                              const float* sampling_loc, const float* attn_weight, const float* grad_output,
                              float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                              int N, int S, int M, int D, int L, int Lq, int P,
                              void* workspace, size_t workspace_bytes, void* stream);
/* The same with a bf16 `value` (raw bf16 bits; mixed-precision training): each value is widened exactly to fp32 as it is loaded
 * and every later instruction is mvg_msda_backward_det_f32's, so all three fp32 outputs equal that function's on the
 * upcast value, bit for bit.  Same shape limits and workspace. */
int mvg_msda_backward_det_bf16(const void* value, const int64_t* shapes_host, const int64_t* starts_host,
                               const float* sampling_loc, const float* attn_weight, const float* grad_output,
                               float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Balanced form of the deterministic backward: the same tile-binned, fixed-point chain with the reduce step launched over
 * (bin, chunk) work items.  The entries of a bin are cut into chunks of at most `chunk` entries and every chunk is one
 * workgroup, so a bin that holds tens of thousands of samples (training with the matcher: every unmatched query projects to
 * one pixel per view) is spread over many CUs instead of being walked by one workgroup; a bin of at most `chunk` entries takes
 * the det path unchanged.  Contract:
 *   - grad_value, grad_sampling_loc and grad_attn_weight are BIT-IDENTICAL to mvg_msda_backward_det_f32 / _bf16 for every
 *     input those accept and every legal chunk: grad_value is a sum of int32 contributions in 64-bit integers (any partition
 *     of a bin gives the same integer; the conversion is the same expression), the other two are computed per sample.
 *   - no host read-back and a data-independent launch: the reduce grid is the host's bound of the item count, at most
 *     N * bins_per_image + floor(N * Lq * M * L * P / chunk) workgroups; the item table is built on the device and workgroups
 *     past the real count exit at once.  Capturable in a HIP graph and replayable on other data in the same buffers.
 *   - the interior pixels of a split bin are summed with 64-bit integer atomics in a region of the workspace that the call
 *     zeroes itself (nothing depends on what the workspace held) and converted once; empty bins still write their zeros.
 *   - work item k of head m is workgroup k * M + m: a workgroup's index modulo M is its head, as in the det form.
 *   - chunk: per call (frozen into a captured graph), 0 = the library default, otherwise a positive multiple of 256 (one
 *     workgroup pass); anything else: MVG_E_BADARG, and mvg_msda_backward_bal_workspace returns 0.
 *   - same availability as the det form: mvg_msda_backward_bal_workspace is 0 exactly where mvg_msda_backward_det_workspace
 *     is (for a legal chunk), and at least that function's size otherwise. */
size_t mvg_msda_backward_bal_workspace(int N, int S, int M, int D, int L, int Lq, int P, const int64_t* shapes_host, int chunk);
int mvg_msda_backward_bal_f32(const float* value, const int64_t* shapes_host, const int64_t* starts_host,
                              const float* sampling_loc, const float* attn_weight, const float* grad_output,
                              float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                              int N, int S, int M, int D, int L, int Lq, int P,
                              void* workspace, size_t workspace_bytes, void* stream, int chunk);
int mvg_msda_backward_bal_bf16(const void* value, const int64_t* shapes_host, const int64_t* starts_host,
                               const float* sampling_loc, const float* attn_weight, const float* grad_output,
                               float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P,
                               void* workspace, size_t workspace_bytes, void* stream, int chunk);

/* ---- stage entry points of the decoder layer ------------------------------------------ */


/* all L levels in one launch: src_nchw_host = HOST array of L device pointers to the (N_img,C,H_l,W_l) maps */
int mvg_pack_pyramid(const float* const* src_nchw_host, void* feat, int dtype, int N_img, int C, const int64_t* shapes_host,
                     const int64_t* starts_host, int L, int S, void* stream);

/* A.1 + A.2 projection (dq_decoder.py:331-397,570-573; cameras.py:167-217): X (B,Lq,3) mm,
 * cams (V*B, MVG_CAM_STRIDE) -> r (V*B,Lq,2) normalised network-image coords,
 * ref_lvl (V*B,Lq,L,2) = r * (W_l,H_l)/(W_l-1,H_l-1), inside (V*B,Lq) uint8.
 * shapes_host: L x (H,W) int64 on the host. */
int mvg_project(const float* X, const float* cams, const int64_t* shapes_host, int L,
                float* r, float* ref_lvl, uint8_t* inside, int V, int B, int Lq, void* stream);

/* A.3 step 1 (projattn.py:134,148-153,180): bilinear ref-point features of every level
 * + (tgt+query_pos) -> ain (V*B*Lq*L, C) in `dtype`.  feat (V*B,S,C) `dtype`;
 * ref_lvl (V*B,Lq,L,2); x (B,Lq,C) f32; shapes/starts host int64 arrays (L). */
int mvg_gather_ref(const void* feat, int dtype, const float* ref_lvl, const float* x,
                   const int64_t* shapes_host, const int64_t* starts_host, void* ain,
                   int V, int B, int Lq, int L, int S, int C, void* stream);

/* Dense projection out[M,N] = act(A[M,K] @ W[N,K]^T + bias[N]) (* rowmask[M]) on MFMA.
 * a_dtype / w_dtype / out_dtype: MVG_F32 or MVG_BF16 (weights must match the compute
 * dtype: bf16 weights -> bf16 MFMA, A converted on load; f32 weights -> fp32 products, formed either as six bf16 MFMAs on
 * operands split into three bf16 parts (default; fp32 accuracy, not bitwise an fmaf chain; Inf / > 3.39e38 inputs give NaN)
 * or as v_mfma_f32_32x32x2_f32 (mvg_set_tuning("f32_split", 0): bitwise an fp32 fmaf chain)).
 * relu: 0/1.  rowmask: NULL or uint8 (M).  lda/ldc in elements.
 * Per element: x = acc + bias; relu; rowmask ? x : 0; rounding to out_dtype (bf16: nearest even).  relu is torch.relu's: a NaN
 * stays a NaN; a non-finite value of A reaches its own output row only; a row with rowmask 0 is +0 whatever its inputs hold. */
int mvg_linear(const void* A, int a_dtype, int lda, const void* W, int w_dtype,
               const float* bias, void* out, int out_dtype, int ldc,
               const uint8_t* rowmask, int relu, int M, int N, int K, void* stream);

/* mvg_linear (fp32) over rows in a processing order, skipping tiles the consumer masks: tile row i works on row order[m0 + i] of
 * A / out; a tile none of whose rows has inside[row] != 0 writes `masked_row` (N floats, what the same kernel computes for such
 * a row) to all its rows without arithmetic.  The per-view output projection and pose MLP of the fp32 path (projattn.py:203,
 * dq_decoder.py:585-586, 673-690): pairs outside the image -- a third of them at cfg-2 -- cost a broadcast instead of three GEMMs. */
int mvg_linear_ordered(const float* A, int lda, const float* W, const float* bias, float* out, int ldc,
                       const uint8_t* rowmask, int relu, int M, int N, int K, const int32_t* order,
                       const uint8_t* inside, const float* masked_row, void* stream);



/* The same with the bias gradient and the sum over the slices: dW (N, K) = dY^T X and, when db is not NULL, db (N) = the column sums
 * of dY (what autograd's Linear backward returns for weight and bias, lib/models/dq_decoder.py:659-717 under run/train_3d.py).
 * `partial` (splits, N, K) and `partial_db` (splits, N) are workspaces; a second small launch adds them in slice order
 * (deterministic; dW equals mvg_linear_wgrad_f32's partials summed slice 0 first). */
int mvg_linear_wgrad_bias_f32(const float* dY, int ldy, const float* X, int ldx, float* partial, float* partial_db, float* dW, float* db,
                              int rows, int N, int K, int splits, void* stream);
/* The same for bf16 dY and X (raw bf16 bits; 8-byte aligned, N, K, ldy, ldx multiples of 4) with fp32 dW / db: one bf16 MFMA per
 * 16 k on the same tiles, slices and k order; on the same values the result equals mvg_linear_wgrad_bias_f32's bit for bit (the
 * split form's lower parts are zero).  rows may be 0 (dW and db are then zero). */
int mvg_linear_wgrad_bias_bf16(const void* dY, int ldy, const void* X, int ldx, float* partial, float* partial_db, float* dW, float* db,
                               int rows, int N, int K, int splits, void* stream);

/* mvg_linear with the activation formed as A + A2 on load (A2: fp32, same shape and leading dimension as A, or NULL):
 * the query term of the first layer, Linear(tgt + query_pos) (dq_decoder.py:580 `with_pos_embed` + projattn.py:180-181),
 * without a separate elementwise pass over the two (B*Lq, 256) tensors. */
int mvg_linear_sum(const void* A, const void* A2, int a_dtype, int lda, const void* W, int w_dtype, const float* bias,
                   void* out, int out_dtype, int ldc, const uint8_t* rowmask, int relu, int M, int N, int K, void* stream);

/* A.3 steps 3-6 fused (projattn.py:180-200): oa (V*B*Lq*L, 192) f32 = Linear outputs
 * [sampling_offsets(128) | attention_weights(64)] per level row; reinterpretation,
 * softmax(L*P), locations (ref_lvl (V*B*Lq,L,2) + offset/(W,H)) and multi-scale sampling of
 * value (V*B,S,256).  M=8, D=32, P=8.
 * samp (V*B*Lq, 256) in `dtype`. */
int mvg_msda_fused(const void* value, int dtype, const float* oa, const float* ref_lvl,
                   const int64_t* shapes_host, const int64_t* starts_host, void* samp,
                   int N_img, int Lq, int L, int S, void* stream);

/* G-sampling in fp32 (the reference's arithmetic; replaces mvg_gather_ref + the (V*Lq*L x 256 x 192) mvg_linear +
 * mvg_msda_fused of the fp32 path): value (V*B,S,256) f32 pixel-major; G (V*B*S, 192) f32 = feat @ [Woff; Wattn]^T with the
 * columns in mvgformer_amd.ops.gsamp_column_order (no bias); xw (B*Lq, 192) f32 = (tgt+query_pos) @ W^T + b, same column
 * order; samp (V*B*Lq, 256) f32.  Bilinear sampling commutes with the Linear, so the results equal the gather-then-Linear
 * form to fp32 rounding.  pair_mask / order (or NULL) as in mvg_msda_gsamp: masked pairs are zero-filled without being
 * sampled (the consumer multiplies exactly these rows by the in-image mask, dq_decoder.py:585-586), slot i of the launch
 * computes pair order[i].  M=8, D=32, P=8, L<=4. */
int mvg_msda_gfused_f32(const float* value, const float* G, const float* xw, const float* ref_lvl,
                        const int64_t* shapes_host, const int64_t* starts_host, float* samp,
                        const uint8_t* pair_mask, const int32_t* order,
                        int N_img, int Lq, int L, int S, int B, void* stream);

/* Several of the two products above over the SAME packed pyramid in ONE launch (round 5): job j is a value projection into head
 * planes (planes[j] != 0: N[j] = 256, bias[j] required, out[j] = vh) or a G product (planes[j] == 0: N[j] = 192, bias ignored,
 * out[j] = G row-major).  The host arrays hold njobs (1..8) entries.  An XCD's workgroups are divided among the jobs and sweep
 * its row tiles together, so the pyramid is fetched through the fabric once per launch instead of once per product; every
 * output is bit-identical to the single-product entry points (same kernel body).  slots_per_xcd: persistent workgroups per
 * XCD (0 = the default: all 64 resident ones; fewer leave CU room for kernels that run next to the launch).
 * projattn.py:169,180-181 for all layers. */
int mvg_pyramid_group_ws(const void* feat, int n_img, int S, int njobs, const void* const* Wf, const float* const* bias,
                         void* const* out, const int* N, const int* planes, int slots_per_xcd, void* stream);
int mvg_msda_gsamp(const void* vh, const void* G, const float* xw, const float* ref_lvl,
                   const int64_t* shapes_host, const int64_t* starts_host, void* samp,
                   const uint8_t* pair_mask, const int32_t* order,
                   int N_img, int Lq, int L, int S, int B, void* stream);

/* Processing order for mvg_msda_gsamp: per image, the Lq (image, query) pairs counting-sorted by the Morton code of
 * the level-0 cell block of their reference point, pairs with inside == 0 last.  order (N_img*Lq) int32 holds
 * global pair indices (n*Lq + q), a permutation of all of them; it changes where a pair is computed, never its result.
 * inside may be NULL.
 * workspace: device scratch of at least mvg_bin_pairs_workspace(N_img, Lq) bytes (0 for small Lq), or NULL: with it,
 * images with many pairs are sorted by 8 workgroups each (two kernels) instead of one.
 * Layout: with the workspace (>= 8192 pairs per image) the in-image pairs of ALL images come first, image by image, then the
 * pairs with inside == 0, image by image -- consumers that skip the latter then find them in one run at the end of their launch
 * instead of one run per image; without it every image's Lq entries are [its in-image pairs | its other pairs]. */
size_t mvg_bin_pairs_workspace(int N_img, int Lq);
int mvg_bin_pairs(const float* ref_lvl, const uint8_t* inside, const int64_t* shapes_host, int L, int32_t* order,
                  int N_img, int Lq, void* workspace, size_t workspace_bytes, void* stream);

/* A.4 (dq_decoder.py:770): mean over views of attn (V,B*Lq,C) `dtype` -> (B*Lq,C) `dtype`. */
int mvg_mean_views(const void* attn, int dtype, void* out, int V, int rows, int C, void* stream);

/* y = LayerNorm(res + h) * gamma + beta, eps 1e-5 (norm2 / norm3, dq_decoder.py:776-778,
 * mvp_decoder.py:94-98).  res f32 (rows,C); h `h_dtype`; y f32. */
int mvg_add_layernorm(const float* res, const void* h, int h_dtype, const float* gamma,
                      const float* beta, float* y, int rows, int C, void* stream);

/* A.5 (dq_decoder.py:889-908,596-623): class head + validity.  tgt (B,NQ*J,C) f32,
 * Wc (2,C), bc (2) -> prob (B,NQ,2); valid (B,NQ) uint8 = prob[...,1] > threshold
 * (or the caller-provided `forced_valid` mask when not NULL: training indices);
 * any_valid: 1 int, must be zeroed by the caller; set to 1 if any query is valid. */
int mvg_class_head(const float* tgt, const float* Wc, const float* bc, float threshold,
                   const uint8_t* forced_valid, float* prob, uint8_t* valid, int* any_valid,
                   int B, int NQ, int J, int C, void* stream);

/* last pose_embed layer (N=3): o (rows,3) f32 = h (rows,C) @ W3 (3,C)^T + b3. */
int mvg_rowdot3(const void* h, int h_dtype, const float* W3, const float* b3, float* o,
                int rows, int C, void* stream);

/* Fused bf16 chain per (image, query) row (dq_decoder.py:585-588,659-690):
 *   attn = inside * (samp @ Wp^T + bp)                       (stored: input of the view mean)
 *   o    = W2 relu(W1 relu(W0 attn + b0) + b1) + b2          (dx, dy, confidence logit)
 * samp/attn (rows,256) bf16; Wp,W0,W1 (256,256) bf16; W2 (3,256) f32; biases f32; o (rows,3) f32.
 * Replaces mvg_linear x3 + mvg_rowdot3 of the unfused path; activations stay in LDS.
 * order (rows) i32 or NULL: tile row i of the launch works on row order[i] (mvg_bin_pairs: masked rows last).
 * o_masked (3) f32 or NULL: o of a row with inside == 0 (the MLP of a zero row; obtain it by running this entry
 * point on one masked row).  When given, 64-row tiles without a single in-image row only write attn = 0 and
 * o = o_masked instead of running the chain. */
int mvg_chain_attn_pose(const void* samp, const uint8_t* inside, const void* Wp, const float* bp,
                        const void* W0, const float* b0, const void* W1, const float* b1,
                        const float* W2, const float* b2, void* attn, float* o,
                        const int32_t* order, const float* o_masked, int rows, void* stream);

/* ---- fp32 path as fused kernels (fp32 storage, fp32-accurate products on the fp16 matrix pipe; csrc/f32s.hip) ----------------
 * The reference's arithmetic is fp32 (lib/models/ops/src/cuda/deform_cuda.cu:75 dispatches float / double only; the Linears of
 * lib/models/dq_decoder.py:763-848,659-717 and lib/models/ops/modules/projattn.py:169,180-181,203 are fp32 nn.Linear).  These
 * entry points keep fp32 tensors at every boundary and form every product as three fp16 MFMAs (l*h + h*l + h*h, fp32 accumulate)
 * on operands scaled by a power of two and split into two fp16 parts (x 2^s = h + l: 22 bits of each operand; error against the
 * fp64 product not above an fp32 fmaf chain's, tests/test_hip_parity.py).  Weight operands W*_planes: the weight times 2^scale as
 * two fp16 planes (h, l), each in the MFMA-fragment order of mvg_chain_attn_pose (mvgformer_amd.ops.swizzle_weight), plane p at
 * element offset p * N * K, N padded to a multiple of 256 with zero rows (mvgformer_amd.ops.split_swizzle_weight_h2, which also
 * returns the scale); activation rows are scaled by the kernels (a power of two per row from the row's maximum).  A non-finite
 * input value makes its output row NaN.  The range-safe alternative is the unfused path on mvg_linear's three-part split form. */

/* chain B in fp32 (lib/models/dq_decoder.py:770-778, lib/models/mvp_decoder.py:94-98, dq_decoder.py:889-908): attn (V, B*NQ*J, 256)
 * f32; Wu (256,256), W1 (1024,256), W2 (256,1024), W_next (n_next padded to 256, 256) as planes with their scales; everything else
 * as in mvg_chain_update_ffn_class (n_next: multiple of 32).  32- or 64-row tiles by the row count (both sum a row identically).
 * The FFN's hidden activations carry a scale per (row, 256-column chunk); the residual t1 stays in fp32 registers.  Replaces
 * mvg_mean_views + mvg_linear x 3 (+ the next layer's query-term GEMM) + mvg_add_layernorm x 2 + mvg_class_head of the unfused path. */
int mvg_chain_update_ffn_class_f32h(const float* attn, int V, const float* tgt, const void* Wu, int wu_scale, const float* bu,
                                    const float* g2, const float* be2, const void* W1, int w1_scale, const float* b1, const void* W2,
                                    int w2_scale, const float* b2, const float* g3, const float* be3, const float* Wc, const float* bc,
                                    float threshold, const uint8_t* forced_valid, float* tgt_out, float* prob, uint8_t* valid,
                                    int* any_valid, const float* query_pos, const void* W_next, int wn_scale, const float* b_next,
                                    float* xw_next, int n_next, int B, int NQ, int J, int has_ffn, void* stream);

/* chain A in fp32 (lib/models/dq_decoder.py:585-588,659-690): samp / attn (rows, 256) f32, o (rows, 3) f32; Wp, W0, W1 planes of the
 * (256, 256) weights with their scales; W2 (3, 256) f32; order / o_masked as in mvg_chain_attn_pose (o_masked: this entry point run
 * on one masked row).  Activation rows are scaled between the stages (row maximum over the 8 wavefronts through LDS); attn is
 * stored as the exact fp32 result of its stage.  Replaces mvg_linear_ordered x 3 + mvg_rowdot3 of the unfused fp32 path. */
int mvg_chain_attn_pose_f32h(const float* samp, const uint8_t* inside, const void* Wp, int wp_scale, const float* bp, const void* W0,
                             int w0_scale, const float* b0, const void* W1, int w1_scale, const float* b1, const float* W2,
                             const float* b2, float* attn, float* o, const int32_t* order, const float* o_masked, int rows,
                             void* stream);

/* value = feat @ Wv^T + bv  (rows, 256)  and  G = feat @ Wg^T  (rows, n_g)  in one pass over the packed fp32 pyramid feat
 * (rows, 256): the value projection of projattn.py:169 and the pyramid side of the offsets / logits Linear (projattn.py:180-181
 * through Linear(bilinear(feat) + x) = bilinear(feat W^T) + (x W^T + b), see mvg_msda_gfused_f32).  n_g: multiple of 32, <= 256. */
int mvg_pyramid_f32h(const float* feat, const void* Wv_planes, int wv_scale, const float* bv, const void* Wg_planes, int wg_scale,
                     float* value, float* G, int64_t rows, int n_g, void* stream);

/* Fused bf16 chain per joint token (dq_decoder.py:770-778, mvp_decoder.py:94-98, dq_decoder.py:889-908):
 *   t1 = LN2(tgt + Wu mean_v(attn_v) + bu);  tgt' = LN3(t1 + W2 relu(W1 t1 + b1) + b2) (has_ffn) else t1;
 *   prob = mean_j sigmoid(Wc tgt' + bc);  valid = prob[...,1] > threshold (or forced_valid).
 * attn (V, B*NQ*J, 256) bf16; tgt/tgt_out (B*NQ*J, 256) f32; Wu (256,256), W1 (1024,256), W2 (256,1024) bf16
 * in the fragment order of csrc/chain.hip (mvgformer_amd.ops.swizzle_weight); LN params / biases f32;
 * any_valid must be zeroed by the caller.  Replaces mean_views + 3 linears + 2 add_layernorm + class_head.
 * Optional tail (W_next != NULL): xw_next (B*NQ*J, n_next) f32 = (tgt' + query_pos) @ W_next^T + b_next, the query
 * term of the NEXT layer's offsets/logits Linear (the xw operand of mvg_msda_gsamp), computed while the rows are in
 * LDS.  W_next: (256,256) bf16 fragment order, rows >= n_next zero; b_next: 256 f32 (zero padded); query_pos
 * (B*NQ*J, 256) f32 or NULL; n_next <= 256, multiple of 4.
 * attn_inside (V, B*NQ*J) u8 or NULL: the in-image flags mvg_chain_attn_pose was given.  Rows of attn with flag 0 are zero
 * by construction; with the flags the view mean does not read them (same sums, a third fewer bytes at cfg-2). */
int mvg_chain_update_ffn_class(const void* attn, int V, const float* tgt, const void* Wu, const float* bu,
                               const float* g2, const float* be2, const void* W1, const float* b1,
                               const void* W2, const float* b2, const float* g3, const float* be3,
                               const float* Wc, const float* bc, float threshold,
                               const uint8_t* forced_valid, float* tgt_out, float* prob, uint8_t* valid,
                               int* any_valid, const float* query_pos, const void* W_next, const float* b_next,
                               float* xw_next, int n_next, int B, int NQ, int J, int has_ffn, const uint8_t* attn_inside, void* stream);

/* A.6-A.8 (dq_decoder.py:659-717,399-461,119-246,1013-1029; multiview.py:170-269):
 * 2D refinement, view-softmax confidence, un-crop, 5-iteration undistortion, DLT rows,
 * smallest right singular vector, masked scatter.
 * r (V*B,Lq,2); o (V*B,Lq,3) = (dx,dy,conf logit); cams (V*B,STRIDE); valid (B,NQ);
 * any_valid (1 int: if 0, query (0,0) is forced valid, dq_decoder.py:620-623).
 * Outputs: new_ref (B,Lq,3) mm; ref2d, proj2d (B,V,Lq,2) network-image px; zeros for
 * non-valid queries. */
int mvg_triangulate(const float* r, const float* o, const float* cams, const uint8_t* valid,
                    const int* any_valid, float* new_ref, float* ref2d, float* proj2d,
                    int V, int B, int NQ, int J, void* stream);

/* mvg_triangulate + the NEXT layer's mvg_project in one launch: the lanes that solved a (query, joint) problem project
 * its new 3D point (zeros for queries that did not pass, exactly what the next layer receives as reference_points) into
 * all V views -> r_next (V*B,Lq,2), ref_lvl_next (V*B,Lq,L,2), inside_next (V*B,Lq), bit-identical to mvg_project(new_ref). */
int mvg_triangulate_project(const float* r, const float* o, const float* cams, const uint8_t* valid,
                            const int* any_valid, float* new_ref, float* ref2d, float* proj2d,
                            int V, int B, int NQ, int J, const int64_t* shapes_host, int L,
                            float* r_next, float* ref_lvl_next, uint8_t* inside_next, void* stream);

/* ---- live-view table: the same launches on a per-stream subset of the V views ------------------------------------------------
 * view_idx (B, V) i32: the live views of stream b in ascending order, padded with -1; n_live (B) i32: their count, >= 1.  Both on
 * the device (a captured graph addresses them; mvgformer_amd.decoder.DecoderContext.set_live_views fills them).  Each entry point
 * takes its namesake's arguments and the table in front of the stream, and gives -- bit for bit, in the slots of the live views --
 * what the namesake gives when it is run on the live views alone; a dead view is not read (camera record, attn rows, pose outputs).
 * V <= 64 for all six (checked by each; the projection, the bf16 chain and the triangulation keep a stream's live views in a 64-bit
 * mask read from the V entries of its row).  The entries of view_idx must be -1 or in [0, V): the kernels shift and index by them
 * unchecked, DecoderContext.set_live_views builds them on the host.
 *   mvg_project_live                 pairs of a dead view: r = ref_lvl = 0, inside = 0
 *   mvg_mean_views_live              (B: streams of the `rows` rows) live views added in ascending order, divided by n_live[b]
 *   mvg_chain_update_ffn_class_live  the view mean of the row's stream (b = row / (NQ * J)): dead views add +0, divisor 1 / n_live[b];
 *   ..._f32h_live
 *   mvg_triangulate_live             lane `sub` of a problem takes the live views k = sub, sub + 8, ... < n_live[b]: softmax and Gram
 *   mvg_triangulate_project_live     sums see the subset run's operands in its lanes; ref2d / proj2d / r_next / ref_lvl_next /
 *                                    inside_next of dead views are zeros */
int mvg_project_live(const float* X, const float* cams, const int64_t* shapes_host, int L, float* r, float* ref_lvl,
                     uint8_t* inside, int V, int B, int Lq, const int32_t* view_idx, const int32_t* n_live, void* stream);
int mvg_mean_views_live(const void* attn, int dtype, void* out, int V, int B, int rows, int C, const int32_t* view_idx,
                        const int32_t* n_live, void* stream);
int mvg_chain_update_ffn_class_live(const void* attn, int V, const float* tgt, const void* Wu, const float* bu,
                                    const float* g2, const float* be2, const void* W1, const float* b1,
                                    const void* W2, const float* b2, const float* g3, const float* be3,
                                    const float* Wc, const float* bc, float threshold,
                                    const uint8_t* forced_valid, float* tgt_out, float* prob, uint8_t* valid,
                                    int* any_valid, const float* query_pos, const void* W_next, const float* b_next,
                                    float* xw_next, int n_next, int B, int NQ, int J, int has_ffn, const uint8_t* attn_inside,
                                    const int32_t* view_idx, const int32_t* n_live, void* stream);
int mvg_chain_update_ffn_class_f32h_live(const float* attn, int V, const float* tgt, const void* Wu, int wu_scale, const float* bu,
                                         const float* g2, const float* be2, const void* W1, int w1_scale, const float* b1,
                                         const void* W2, int w2_scale, const float* b2, const float* g3, const float* be3,
                                         const float* Wc, const float* bc, float threshold, const uint8_t* forced_valid,
                                         float* tgt_out, float* prob, uint8_t* valid, int* any_valid, const float* query_pos,
                                         const void* W_next, int wn_scale, const float* b_next, float* xw_next, int n_next, int B,
                                         int NQ, int J, int has_ffn, const int32_t* view_idx, const int32_t* n_live, void* stream);
int mvg_triangulate_live(const float* r, const float* o, const float* cams, const uint8_t* valid,
                         const int* any_valid, float* new_ref, float* ref2d, float* proj2d,
                         int V, int B, int NQ, int J, const int32_t* view_idx, const int32_t* n_live, void* stream);
int mvg_triangulate_project_live(const float* r, const float* o, const float* cams, const uint8_t* valid,
                                 const int* any_valid, float* new_ref, float* ref2d, float* proj2d,
                                 int V, int B, int NQ, int J, const int64_t* shapes_host, int L,
                                 float* r_next, float* ref_lvl_next, uint8_t* inside_next,
                                 const int32_t* view_idx, const int32_t* n_live, void* stream);

/* Training path: the refined 2D points ref2d (B, V, Lq, 2; network-image px) -> un-cropped, undistorted
 * original-image px ud (B, V, Lq, 2) (lib/models/dq_decoder.py:414-420, 119-204: inverse crop affine, K^-1, 5 fixed-point
 * iterations, K) and jac (B, V, Lq, 4) = the row-major 2 x 2 Jacobian d(ud) / d(ref2d) of every point (forward mode through the
 * same iterations): the backward of this step is grad_ref2d = jac^T grad_ud.  cams: the packed records, image n = v * B + b. */
int mvg_uncrop_undistort_jac(const float* ref2d, const float* cams, float* ud, float* jac, int V, int B, int Lq, void* stream);

/* The differentiable triangulation of the training path (lib/models/multiview.py:170-228 as called by
 * lib/models/dq_decoder.py:929-967 under autograd), dense over the (B, NQ * J) tokens: X (B, NQ*J, 3) = v0[:3] / v0[3], v0 the
 * eigenvector of the smallest eigenvalue of A^T A, A's rows conf[b,v,t] * (P[b,v,2] * ud[b,v,t,c] - P[b,v,c]) (rows, Gram
 * matrix and Jacobi eigen-solve in fp64).  ud (B, V, Lq, 2), conf (B, V, Lq), Pm (B, V, 3, 4) fp32; valid (B, NQ) uint8: tokens of
 * queries with valid == 0 are skipped and get X = 0 (the reference triangulates the matched queries only).  V <= 32. */
int mvg_dlt_forward(const float* ud, const float* conf, const float* Pm, const uint8_t* valid, float* X, int V, int B, int NQ, int J,
                    void* stream);

/* Its backward: g_ud (B, V, Lq, 2), g_conf (B, V, Lq) from gX (B, Lq, 3); the decomposition is recomputed from the inputs
 * (dL/dG = sym(m v0^T), m = sum_{i != 0} v_i (v_i^T g) / (l0 - l_i); pairs with |l0 - l_i| <= 1e-14 max|l| contribute nothing);
 * zero gradients for skipped tokens. */
int mvg_dlt_backward(const float* ud, const float* conf, const float* Pm, const uint8_t* valid, const float* gX, float* g_ud,
                     float* g_conf, int V, int B, int NQ, int J, void* stream);

/* Batched eigen-decomposition of n symmetric 4x4 fp64 matrices G (n,4,4): evals (n,4) in no particular order, evecs
 * (n,4,4) with the eigenvectors as columns (G v_k = evals_k v_k, v_k = evecs[:, :, k]).  fp64 cyclic Jacobi, one lane
 * per matrix.  Used by the differentiable DLT of the training path (multiview.py:170-228 under autograd): smallest
 * eigenvector of A^T A in the forward, all pairs in the backward. */
int mvg_sym4_eigh(const double* G, double* evals, double* evecs, long n, void* stream);

/* ---- training criterion (csrc/criterion.hip) ------------------------------------------------------------------------------ */
#define MVG_MATCH_KNN 0       /* the K nearest queries of every ground-truth person (matcher.py:232-262)          */
#define MVG_MATCH_MULTIPLE 1  /* every query whose nearest person is closer than a threshold (matcher.py:201-230) */

/* bytes of cost workspace mvg_knn_match needs (0 while the NQ x Gmax fp32 costs fit its 40 KB of LDS) */
size_t mvg_knn_match_workspace(int B, int NQ, int Gmax);

/* Ground-truth matcher of the training step (lib/models/matcher.py:80-262, match_coord_est 'abs', match_coord_gt 'norm') for the
 * whole batch in ONE launch, one workgroup per batch element, nothing read back by the host.  poses (B, NQ*J, 3) fp32 absolute mm;
 * joints_3d (B, Gmax, J, 3) fp32 absolute mm, taken through absolute -> norm -> absolute in fp32 as the reference does;
 * num_person (B,) int32 (num_person_is64 = 0) or int64 (1), clamped to [0, Gmax]; space_size / space_center: 3 HOST floats.
 * cost = 0.01 * L1 over the 3J coordinates.  method MVG_MATCH_KNN: the K smallest-cost queries of every person, pair slot g*K + k
 * (person-major, ascending cost, ties to the lower query index), pair_count[b] = num_person[b] * K, Pmax >= Gmax*K;
 * MVG_MATCH_MULTIPLE: every query whose nearest person (ties to the lower person) costs less than `value`, ascending query order
 * (the reference's torch.where order), Pmax >= NQ.  Outputs: pair_query, pair_gt (B, Pmax) int32, -1 in unused slots; pair_count
 * (B,) int32; matched (B, NQ) uint8 = the union of the matched queries (a query matched to two persons is in two pairs and once
 * here), ready to be the decoder's triangulation filter.  MVG_E_BADARG for Gmax > 64, K > 16, K > NQ, J > 64, value <= 0, a
 * too small Pmax or workspace. */
int mvg_knn_match(const float* poses, const float* joints_3d, const void* num_person, int num_person_is64, const float* space_size,
                  const float* space_center, int method, int K, float value, int B, int NQ, int Gmax, int J, int Pmax,
                  void* workspace, size_t workspace_bytes, int* pair_query, int* pair_gt, int* pair_count, uint8_t* matched,
                  void* stream);

/* mvg_knn_match between predictions with Jp joints per query and a ground truth with Jc joints per person (the Shelf / Campus
 * joint format, lib/models/dq_transformer.py:90-104: the reference gathers the initial poses with convert_joint_format_indices
 * before its matcher).  poses (B, NQ*Jp, 3); joints_3d (B, Gmax, Jc, 3); joint_map: Jc HOST ints, converted joint j is prediction
 * joint joint_map[j]: cost[g][q] = 0.01 * sum_{j < Jc, c} |pose[q][joint_map[j]][c] - gt'[g][j][c]|, j ascending, then c.  The
 * map travels by value in the launch arguments: no device table, no upload, no further launch; a captured graph keeps the map
 * it was captured with, as it keeps K.  joint_map NULL = the identity and requires Jc == Jp: that call IS mvg_knn_match, bit
 * for bit.  Everything else -- norm round trip, tie rules, pair layout, pair_count, matched, workspace -- as mvg_knn_match.
 * MVG_E_BADARG, nothing launched: an entry repeated or outside [0, Jp), Jp or Jc outside [1, 64], NULL with Jc != Jp, and every
 * limit of mvg_knn_match. */
int mvg_knn_match_jm(const float* poses, const float* joints_3d, const void* num_person, int num_person_is64,
                     const float* space_size, const float* space_center, int method, int K, float value, int B, int NQ, int Gmax,
                     int Jp, int Jc, const int* joint_map, int Pmax, void* workspace, size_t workspace_bytes, int* pair_query,
                     int* pair_gt, int* pair_count, uint8_t* matched, void* stream);

/* ---- one-to-one ground-truth matcher (csrc/hungarian.hip) ---------------------------------------------------------------------- */
#define MVG_MATCH_HUNGARIAN      2   /* C = cost_pose * pose + cost_class * class  (matcher.py:175) */
#define MVG_MATCH_HUNGARIAN_DIS  3   /* C = pose                                   (matcher.py:172) */
#define MVG_HUNGARIAN_MAX_G   64
#define MVG_HUNGARIAN_MAX_NQ  4096

/* bytes of cost workspace mvg_hungarian_match needs (0 while the Gmax x NQ fp32 pose costs fit its 40 KB of LDS; 4-byte aligned) */
size_t mvg_hungarian_match_workspace(int P, int NQ, int Gmax);

/* The reference's default matcher (lib/models/matcher.py:80-199, methods 'hungarian' / 'hungarian-dis': scipy's
 * linear_sum_assignment per batch element behind a .cpu()) for P = Lm * B independent problems in ONE launch, one workgroup of
 * 256 lanes per problem, nothing read back, graph-capturable.  Problem p uses the ground truth of batch element p % B: Lm = 1 is
 * the match on the initial poses, Lm = L matches every layer's own outputs.
 *   logits (P, NQ, 2) fp32 or NULL (= logit 1.0 for every query, the reference's construct_output_from_origin); poses
 *   (P, NQ*Jp, 3) fp32 absolute mm; joints_3d (B, Gmax, Jc, 3), num_person (B,), space_size, space_center and joint_map exactly as
 *   for mvg_knn_match_jm (joint_map NULL = the identity, requires Jc == Jp).
 * Costs.  pose[g][q]: the fp32 value mvg_knn_match(_jm) computes (same norm round trip, same summation order, same device
 * function, csrc/match_dev.h: in the round trip n * size + center is one fused multiply-add, as these matchers have always
 * been built; NaN and inf sums become +inf).  class[q], in fp64: p = 1 / (1 + exp(-(double)logits[q][1])),
 *   class[q] = 0.25 (1-p)^2 (-log(p + 1e-8)) - 0.75 p^2 (-log(1 - p + 1e-8))          (matcher.py:151-162, every target class 1).
 * MVG_MATCH_HUNGARIAN: C[g][q] = (double)cost_pose * pose + (double)cost_class * class, each product and the sum rounded on its
 * own; MVG_MATCH_HUNGARIAN_DIS: C[g][q] = (double)pose.  An entry that is NaN or above MVG_LAP_BIG is taken as MVG_LAP_BIG.
 * Solver: the algorithm of mvg_linear_assignment (below), stated for the rectangular problem without padding: rows are the
 * G = clamp(num_person[p % B], 0, Gmax) persons, columns the NQ queries (NQ >= Gmax required); potentials u, v start at 0, rows
 * are inserted in order, steps 1 to 4 as written there, the LOWEST column wins among equal minima, a NaN minimum orders as
 * +inf; the search of row i is a counted loop of at most i + 1 steps and ends at a column without a row.  fp64 throughout, every
 * operation rounded on its own, no atomics: two runs give the same bits.
 * Outputs, every element written by every call: pair_query, pair_gt (P, Gmax) int32: the G pairs in ASCENDING QUERY order
 * (scipy's order for this orientation), -1 in the unused slots; pair_count (P,) = G; matched (P, NQ) uint8; duals (P, Gmax + NQ)
 * fp64 or NULL: the final u[0..Gmax) (0 for rows >= G) followed by v[0..NQ), for verification (u[g] + v[q] <= C[g][q], with
 * equality on the pairs, v = 0 on unmatched columns).
 * MVG_E_BADARG, nothing launched: Gmax > MVG_HUNGARIAN_MAX_G, NQ > MVG_HUNGARIAN_MAX_NQ, NQ < Gmax, P < 1, B < 1, P % B != 0, Jp or
 * Jc outside [1, 64], a bad joint_map, method not 2 or 3, a NULL required pointer, duals not 8-byte aligned, a too small
 * workspace. */
int mvg_hungarian_match(const float* logits, const float* poses, const float* joints_3d, const void* num_person,
                        int num_person_is64, const float* space_size, const float* space_center, int method, float cost_class,
                        float cost_pose, int P, int B, int NQ, int Gmax, int Jp, int Jc, const int* joint_map, void* workspace,
                        size_t workspace_bytes, int* pair_query, int* pair_gt, int* pair_count, uint8_t* matched, double* duals,
                        void* stream);

/* bytes of the (8-byte aligned) workspace of mvg_criterion: the projected ground truth and the per-(layer, batch) partial sums */
size_t mvg_criterion_workspace(int L, int B, int Gmax, int V, int J);

/* SetCriterion (lib/models/multi_view_pose_transformer.py:491-932 with losses labels / cardinality / joints,
 * use_loss_pose_perprojection_2d, loss_joint_type l1, loss_pose_normalize false) for all L decoder layers of one step against
 * ONE pair list (gt_match: every layer uses the match on the initial poses): value and gradients in three launches whatever L,
 * B, Gmax are, fixed-order sums in fp64, no atomics, no host read-back.
 *   logits (L,B,NQ,2), poses (L,B,NQ*J,3) mm, poses_2d (L,B,V,NQ*J,2) network-image px: fp32.
 *   pair_query / pair_gt (B,Pmax), pair_count (B,): as written by mvg_knn_match (entries out of range are ignored).
 *   joints_3d, joints_3d_vis (B,Gmax,J,3); joints_vis (V,B,Gmax,J,2); num_person (B,) int32 / int64.
 *   num_samples: device fp32 scalar (the all-reduced clamp(sum(num_person) / world_size, 1)) or NULL = computed here from
 *   num_person.  cams: packed records (V*B, MVG_CAM_STRIDE); the crop affine of record 0 (view 0, batch element 0) is applied to
 *   every projected ground-truth point, without the clamp of mvg_project.  space_size / space_center: 3 HOST floats.
 * table (L, 8) fp32: loss_ce, class_error, class_recall, class_precision, cardinality_error, loss_pose_perjoint,
 * loss_pose_perprojection_2d (zero if it exceeded 1e5), keep_2d (0 in that case, else 1: the factor of its gradient).
 * grad_logits / grad_poses / grad_poses_2d: d loss_ce / d logits, d loss_pose_perjoint / d poses and d (unguarded 2D loss) /
 * d poses_2d, shaped like the inputs and written densely (zeros for unmatched queries; a query in several pairs gets the sum of
 * their terms in pair order).  The 2D rows keep the reference's order: predictions pair-major, visibility weights view-major
 * (loss.py:260-272).  Limits: NQ <= 4096, Pmax <= 4096, B <= 256, Gmax <= 64, J <= 64. */
int mvg_criterion(const float* logits, const float* poses, const float* poses_2d, const int* pair_query, const int* pair_gt,
                  const int* pair_count, const float* joints_3d, const float* joints_3d_vis, const float* joints_vis,
                  const void* num_person, int num_person_is64, const float* num_samples, const float* cams, const float* space_size,
                  const float* space_center, float pred_conf_threshold, float focal_alpha, float focal_gamma, int L, int B, int NQ,
                  int J, int V, int Gmax, int Pmax, void* workspace, size_t workspace_bytes, float* table, float* grad_logits,
                  float* grad_poses, float* grad_poses_2d, void* stream);

/* mvg_criterion on predictions with Jp joints per query against a ground truth with Jc joints per person (dq_transformer.py:
 * 582-594: the reference gathers 3D poses and 2D points with convert_joint_format_indices before SetCriterion, and the gradient
 * flows back through that gather).  poses (L,B,NQ*Jp,3), poses_2d (L,B,V,NQ*Jp,2); joints_3d, joints_3d_vis (B,Gmax,Jc,3);
 * joints_vis (V,B,Gmax,Jc,2); joint_map: Jc HOST ints as for mvg_knn_match_jm, by value in the launch arguments.  Every loop over
 * joints and every divisor that depends on the joint count uses the Jc converted joints; converted joint j reads the prediction
 * at joint_map[j], and the fp64 sums visit the (query, converted joint, coordinate) elements in the order and with the thread
 * assignment of a mvg_criterion call on gathered predictions (J = Jc): table and gradients equal that call's bit for bit.
 * grad_poses / grad_poses_2d keep the inputs' shapes (Jp joints) and are written densely by every call: the term of converted
 * joint j lands on joint_map[j] (entries are distinct: one writer per element), prediction joints that no entry names get zeros,
 * and so do unmatched queries.  Workspace: mvg_criterion_workspace(L, B, Gmax, V, Jc).  joint_map NULL = the identity and
 * requires Jc == Jp: that call IS mvg_criterion, same launches, same bits.  MVG_E_BADARG, nothing launched: as for
 * mvg_knn_match_jm, and every limit of mvg_criterion. */
int mvg_criterion_jm(const float* logits, const float* poses, const float* poses_2d, const int* pair_query, const int* pair_gt,
                     const int* pair_count, const float* joints_3d, const float* joints_3d_vis, const float* joints_vis,
                     const void* num_person, int num_person_is64, const float* num_samples, const float* cams,
                     const float* space_size, const float* space_center, float pred_conf_threshold, float focal_alpha,
                     float focal_gamma, int L, int B, int NQ, int Jp, int Jc, const int* joint_map, int V, int Gmax, int Pmax,
                     void* workspace, size_t workspace_bytes, float* table, float* grad_logits, float* grad_poses,
                     float* grad_poses_2d, void* stream);

/* ---- optimizer step (csrc/optim.hip) -------------------------------------------------------------------------------------- */
#define MVG_OPTIM_CHUNK 4096          /* elements of one tensor that one workgroup handles                                  */
#define MVG_OPTIM_MAX_GROUPS 64
#define MVG_OPTIM_TENSOR_WORDS 6      /* 8-byte words per tensor record                                                      */
#define MVG_OPTIM_GROUP_WORDS 6       /* doubles per group record                                                            */
#define MVG_OPTIM_STATE_HEADER 64     /* bytes of the state block in front of the per-group results                          */
#define MVG_OPTIM_STATE_PER_GROUP 16

/* bytes of the (8-byte aligned) workspace of mvg_optim_step: one fp64 partial sum per chunk */
size_t mvg_optim_workspace(int n_chunks);

/* One optimizer step over every parameter tensor of a model: clip_grad_norm_(max_norm) followed by Adam / AdamW
 * (lib/core/function.py:167-178), in at most three launches, without memset, copy or atomics, nothing read back.  Unlike the
 * other entry points this one updates memory it is handed: p, exp_avg, exp_avg_sq, grad and the state block.  All tables are in
 * DEVICE memory, 8-byte aligned:
 *   tensor_table  n_tensors records of 6 x 8 bytes: pointers p, grad, exp_avg, exp_avg_sq (fp32, n elements each), int64 n,
 *                 int64 group.  Pointers aligned to 16 bytes take the vector path, others the scalar one.
 *   chunk_table   n_chunks records {int32 tensor, int32 index}: elements [index * MVG_OPTIM_CHUNK, min(n, (index + 1) *
 *                 MVG_OPTIM_CHUNK)) of that tensor; every element of every tensor in exactly one chunk (an empty tensor in none).
 *   group_table   n_groups (1 .. MVG_OPTIM_MAX_GROUPS) records of 6 doubles: lr, beta1, beta2, eps, weight_decay, decoupled
 *                 (0: Adam, the decay is added to the gradient; 1: AdamW, p *= 1 - lr * weight_decay).
 *   state         MVG_OPTIM_STATE_HEADER + n_groups * MVG_OPTIM_STATE_PER_GROUP bytes, zeroed once by the caller: int64 step
 *                 count at byte 0 (the only field that persists), fp64 total norm at 8, fp32 clip coefficient at 16, int32 skip
 *                 at 20, fp32 loss at 24, then per group fp32 {lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - lr * weight_decay, 0}.
 * loss: device fp32 scalar or NULL; with it the step is skipped unless loss > 0 (a NaN skips): nothing is written to p, exp_avg,
 * exp_avg_sq and the count stays.  max_norm <= 0: no clipping.  The gradient is left multiplied by the clip coefficient, or
 * zeroed if zero_grad (also on a skipped step).  norm_out: device fp32 scalar or NULL, the total norm before clipping.  Sums are
 * fp64 in a fixed order (a function of the tables alone); the update is fp32 in torch.optim.Adam's order of operations.
 * MVG_E_BADARG for bad counts, unaligned tables, a short state block or workspace. */
int mvg_optim_step(const void* tensor_table, int n_tensors, const void* chunk_table, int n_chunks, const void* group_table,
                   int n_groups, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes, const float* loss,
                   float max_norm, int zero_grad, float* norm_out, void* stream);

/* ---- derived bf16 operands of the bf16 training path (csrc/operands.hip) ------------------------------------------------- */
#define MVG_OPERANDS_TILE 64          /* one workgroup converts one 64 x 64 tile                                             */
#define MVG_OPERANDS_RECORD_WORDS 8   /* 8-byte words per source-matrix record                                               */

/* Rewrites, in one launch, the bf16 copy and / or the transposed bf16 copy of every fp32 matrix of a table: what the bf16
 * training path multiplies by, refreshed on the device right behind mvg_optim_step (also inside a HIP graph).  Both tables are
 * in DEVICE memory, 8-byte aligned:
 *   record_table  n_records records of 8 x 8 bytes: src (fp32, row-major N x K), int64 N, K, src_ld (elements), dst (bf16
 *                 row-major N x K, or NULL), int64 dst_ld, dstT (bf16 K x N, or NULL), int64 dstT_ld.  A concatenated weight is
 *                 several records whose dst / dstT point into one buffer (a row offset in dst, a column offset in dstT).
 *   tile_table    n_tiles records {int32 record, int32 tile}: tile t of a record covers rows [64 * (t / ceil(K / 64)), + 64) and
 *                 columns [64 * (t % ceil(K / 64)), + 64) of its source; every tile of every record exactly once.
 * Round to nearest even with the bits of torch's fp32 -> bf16 cast (a NaN becomes 0x7FC0).  16-byte accesses where a whole tile
 * lies inside the matrix and the pointer and leading dimension allow them, element accesses otherwise: the stored value does not
 * depend on the path.  Ordinary stores only; nothing outside the destinations is written, nothing is read back.  n_tiles == 0
 * launches nothing.  MVG_E_BADARG for negative counts, NULL or unaligned tables. */
int mvg_refresh_operands(const void* record_table, int n_records, const void* tile_table, int n_tiles, void* stream);

/* ---- query self-attention (csrc/mha.hip) ------------------------------------------------------------------------------------ */
/* The attention of nn.MultiheadAttention between its in- and out-projection (DQDecoderLayer.self_attn with init_self_attention,
 * dq_decoder.py:281-283,532-539), flash-style: no Lq x Lq matrix in memory, online softmax with a running maximum and sum per
 * query row.  q, k, v: (B, Lq, C) `dtype` with element strides (Lq * ld, ld, 1), ld = ldq / ldk / ldv >= C -- head h in columns
 * 32 h .. 32 h + 31, no transposed copies; so the three may be column blocks of one wider projection output.  out (B, Lq, C)
 * `dtype`, contiguous:  out[b,i,h,:] = sum_j softmax_j(q[b,i,h] . k[b,j,h] / sqrt(32)) v[b,j,h,:]; nothing crosses b.
 *   MVG_BF16: bf16 MFMA products with fp32 accumulation; scores, maximum, sum and rescale fp32; P rounded to bf16 only as the
 *             operand of P V; out rounded once.
 *   MVG_F32 : fp32 MFMA products (k-ordered fp32 fma chains: the reference's arithmetic class, valid at every input range).
 * Finite inputs only (a NaN / Inf spreads over every row that reads it); finite results for any finite scores, rows of equal
 * scores included.  One launch, no workspace, no atomics, a fixed reduction order: bit-identical from run to run, and rows of one
 * batch element do not depend on the others.  MVG_E_BADARG, nothing launched: C != 256, M != 8, B or Lq < 1, B > 65535,
 * Lq > 2^24, a NULL or not 16-byte aligned pointer, ld < C or not a multiple of 16 bytes. */
int mvg_self_attention(const void* q, const void* k, const void* v, void* out, int ldq, int ldk, int ldv, int B, int Lq, int C, int M,
                       int dtype, void* stream);

/* mvg_self_attention for training: the same kernel and, with p_drop == 0, the same bits in `out`, plus
 *   lse (B, 8, Lq) fp32:  lse[b,h,i] = ln sum_j exp(q[b,i,h] . k[b,j,h] / sqrt(32)) -- what the backward recomputes P from; finite
 *       for finite inputs (the row sum is >= 1);
 *   attention dropout:    out = (Z o P) v with Z = keep / (1 - p_q); the row sum and lse come from the undropped P, as in
 *       F.multi_head_attention_forward.  p_drop is quantised to p_q = round(256 p_drop) / 256 (at most 255 / 256): 8 bits per
 *       decision, the scale is that of the quantised value.  keep is a stateless function of (*seed, b, head, query, key) and of
 *       nothing else -- mvg_self_attention_dropout_mask writes it out.  seed points to DEVICE memory (8-byte aligned) and is read
 *       by the kernel when it runs: a captured graph sees the value of each replay.  It may be NULL when p_drop == 0.
 * MVG_E_BADARG, nothing launched: everything mvg_self_attention refuses, a NULL lse, p_drop outside [0, 1) or NaN, p_drop > 0
 * with a NULL or misaligned seed. */
int mvg_self_attention_train(const void* q, const void* k, const void* v, void* out, float* lse, int ldq, int ldk, int ldv, int B, int Lq,
                             int C, int M, int dtype, float p_drop, const uint64_t* seed, void* stream);

/* bytes of mvg_self_attention_backward's workspace (delta, (B, 8, Lq) fp32); 0 for a B or Lq it refuses */
size_t mvg_self_attention_backward_workspace(int B, int Lq);

/* Gradients of mvg_self_attention_train's `out` with respect to q, k, v, flash-style: P is recomputed from q, k and lse, no
 * Lq x Lq matrix in memory.  q, k, v, lse, p_drop, seed: what the forward was given / wrote; out, dout (B, Lq, C) `dtype`,
 * contiguous (out as the forward stored it: in bf16 the rounded one).  dq, dk, dv (B, Lq, C) `dtype` with row strides lddq,
 * lddk, lddv >= C (element strides (Lq * ld, ld, 1)): d[q; k] can be written as the column blocks of one (B * Lq, 512) tensor.
 *   delta = rowsum(dout o out);  dv = (Z o P)^T dout;  dP = dout v^T;  dS = P o (Z o dP - delta) / sqrt(32);  dq = dS k;
 *   dk = dS^T q
 * in three launches (delta; dq with the query on the lane; dk and dv with the key on the lane), each of the two large ones
 * recomputing S and dP.  Every output element has one writer, the reduction order is fixed, there are no atomics and no
 * hand-off between workgroups: bit-identical from run to run, independent of the other batch elements, capturable.
 *   MVG_BF16: q, k, v, out, dout bf16; Z o P and dS rounded to bf16 only as MFMA operands; lse, delta, P, dP, dS fp32; dq, dk,
 *             dv rounded once on store.          MVG_F32: fp32 MFMA chains, the forward's arithmetic class.
 * workspace: at least mvg_self_attention_backward_workspace(B, Lq) bytes, 4-byte aligned.  MVG_E_BADARG, nothing launched:
 * everything mvg_self_attention_train refuses, for dq / dk / dv and their strides what it refuses for q / k / v, a NULL or
 * misaligned out / dout / lse, a NULL or too small workspace. */
int mvg_self_attention_backward(const void* q, const void* k, const void* v, const void* out, const void* dout, const float* lse, void* dq,
                                void* dk, void* dv, int ldq, int ldk, int ldv, int lddq, int lddk, int lddv, int B, int Lq, int C, int M,
                                int dtype, float p_drop, const uint64_t* seed, void* workspace, size_t workspace_bytes, void* stream);

/* The keep mask of the attention dropout as bytes, mask (B, 8, Lq, Lq) uint8 (1 = kept), from the device function the three
 * training kernels call: a test and debugging aid.  p_drop == 0 writes ones.  MVG_E_BADARG: Lq > MVG_MHA_MASK_MAX_LQ, B or
 * Lq < 1, B > 65535, a NULL mask, p_drop / seed as in mvg_self_attention_train. */
#define MVG_MHA_MASK_MAX_LQ 1024
int mvg_self_attention_dropout_mask(unsigned char* mask, int B, int Lq, float p_drop, const uint64_t* seed, void* stream);

/* ---- serving post-processing (csrc/nms.hip) -------------------------------------------------------------------------------- */
#define MVG_NMS_MAX_N 2048            /* candidates rows per batch element                                                    */
#define MVG_NMS_MAX_J 32

/* bytes of the (8-byte aligned) workspace of mvg_pose_nms: per batch element the candidate count, rank -> row, the fp64 distance
 * limits and the N x ceil(N / 64) 64-bit words of the closeness matrix.  Monotone in N; 0 for shapes mvg_pose_nms rejects. */
size_t mvg_pose_nms_workspace(int B, int N, int J);

/* Classification filter + nearby-joints NMS of the packed predictions (run/validate_3d.py:228-234, lib/core/nms.py:210-283) for
 * the whole batch in THREE launches (rank, closeness bit matrix, greedy pass + gather), fixed shapes, nothing read back by the
 * host, no floating-point atomics, bit-reproducible: it can be captured in the HIP graph of the decoder forward.
 *   pred (B, N, J, 5) fp32 contiguous, rows [x, y, z, flag, score]; every batch element on its own.
 *   Candidates: row n iff pred[b, n, 0, 3] >= 0 (the flag as given, the threshold compare is not redone); score pred[b, n, 0, 4].
 *   limit_a = sqrt(sum_c (max_j k[a,j,c] - min_j k[a,j,c])^2) * dist_thr and
 *   close[a, c] = #{ j : sqrt((dx^2 + dy^2) + dz^2) < limit_a } > num_nearby_joints_thr in fp64 from the fp32 inputs, every
 *   multiply and add rounded on its own, correctly rounded sqrt: numpy's arithmetic, so the matrix is the reference's bit for bit
 *   (not symmetric: the limit belongs to the row pose; a NaN coordinate gives a NaN limit as np.max / np.min do).
 *   Caveat: as built, dy^2 and dz^2 enter their sums unrounded (fused multiply-add; csrc/exact_dev.h, CONTRACTION), which is the
 *   same value while those squares are exact in fp64, i.e. while a coordinate difference has at most 26 significant bits.
 *   Greedy pass in visiting order = descending score, among equal scores the HIGHER row first
 *   (np.argsort(scores, kind="stable")[::-1]; the reference's default argsort is unstable, its order among tied scores is
 *   unspecified and coincides with this rule where numpy falls back to insertion sort, N <= 16): a candidate that is already
 *   ignored is skipped; best = the member of its row with the highest score, among equal scores the LOWEST row (np.argmax); if
 *   best is not ignored it is appended to the keep list and the whole row is ignored from then on.  A candidate whose own row is
 *   empty (zero extent: 0 < 0 is false; a NaN limit) is visited, counted in count[b, 1] and keeps / suppresses nothing (the
 *   reference raises inside np.argmax there).
 *   max_dets > 0 and more poses kept: the max_dets best scored kept poses in descending score, among equal scores the later keep
 *   position first (np.argsort(scores[keep], kind="stable")[-1:-max_dets-1:-1]).
 * Outputs: keep (B, N) int32 kept row indices in keep order, -1 behind the count; count (B, 2) int32 [kept, candidates skipped
 * for an empty neighbourhood]; dets (B, dets_rows, J, 5) fp32 or NULL: the kept rows gathered in keep order (the first dets_rows
 * of them), rows behind the count are 0 with flag -1.  Every element of keep, count and dets is written by every call; of the
 * workspace only what the same call wrote is read.  stream: a hipStream_t.
 * MVG_E_BADARG, and nothing launched, for dist_thr <= 0 (or NaN), num_nearby_joints_thr < 0 or >= J, J > MVG_NMS_MAX_J,
 * N > MVG_NMS_MAX_N, B or N or J < 1, dets_rows < 1 or > MVG_NMS_MAX_N with dets given, a NULL pred / keep / count, a NULL,
 * unaligned or too small workspace. */
int mvg_pose_nms(const float* pred, int B, int N, int J, double dist_thr, int num_nearby_joints_thr, int max_dets, void* workspace,
                 size_t workspace_bytes, int* keep, int* count, float* dets, int dets_rows, void* stream);

/* ---- validation scoring behind the NMS (csrc/evalacc.hip) ------------------------------------------------------------------- */
#define MVG_EVAL_MAX_R 2048           /* rows of dets per batch element                                                        */
#define MVG_EVAL_MAX_J 32
#define MVG_EVAL_MAX_G 64             /* person slots of the ground truth, actors of the PCP counters                          */
#define MVG_EVAL_MAX_B 256
#define MVG_EVAL_STATE_WORDS 8        /* int64 state block: n_entries, total_gt, frames, overflow, kept_rows, match_gt,
                                       * empty_frame (1 + the first frame that has an annotated actor and no row; 0: none), 0 */

/* Ground-truth matching of Panoptic.evaluate (lib/dataset/panoptic.py:497-556) on the device, accumulated over calls: TWO launches,
 * fixed shapes, nothing read back, integer LDS atomics only, bit-reproducible; can be captured in a HIP graph behind mvg_pose_nms.
 *   dets (B, R, J, 5) fp32 rows [x, y, z, flag, score] and count (B, 2) int32 or NULL as mvg_pose_nms leaves them: row i of element
 *   b takes part iff dets[b, i, 0, 3] >= 0 and (count == NULL or i < count[b, 0]).
 *   joints_3d (B, Gmax, J, 3) fp32, joints_3d_vis (B, Gmax, J) fp32 (visible iff > 0), num_person (B) int32 (clamped to [0, Gmax]).
 *   An element with num_person == 0 appends nothing and adds nothing to total_gt.  Every other element appends, per participating
 *   row in row order, mean_g = sum_j (dist(row_j, gt_g_j) * w_j) / sum_j w_j (w = 1 for a visible joint, else 0; fp64 from the fp32
 *   inputs, (dx^2 + dy^2) + dz^2, correctly rounded sqrt, joints in order; 0 / 0 = NaN for a person without visible joint; the
 *   caveat of mvg_pose_nms on dy^2 and dz^2 holds for every distance of this call and of mvg_eval_pcp) for
 *   every g < num_person, takes the FIRST minimum over g with NaN ordered as +inf, and writes mpjpe = that mean as computed,
 *   score = the row's score, gt_id = total_gt before this element + g.  Entries go to mpjpe / score / gt_id (capacity each) at the
 *   cursor state[0], elements in batch order; an entry at or past `capacity` is not written.  After every element has read the
 *   state, a one-workgroup launch adds the entries to state[0] (also past the capacity), sum(num_person) to state[1], B to
 *   state[2], the participating rows of ALL elements to state[4], and sets state[3] = 1 when state[0] > capacity.
 * MVG_E_BADARG, and nothing launched, for B, R, J or Gmax < 1 or above their MVG_EVAL_MAX_*, capacity < 1, a NULL pointer other
 * than count, an output or state pointer that is not 8-byte aligned. */
int mvg_eval_match(const float* dets, const int* count, const float* joints_3d, const float* joints_3d_vis, const int* num_person, int B,
                   int R, int J, int Gmax, double* mpjpe, double* score, int64_t* gt_id, int64_t capacity, int64_t* state,
                   void* stream);

/* PCP counters of Shelf.evaluate / Campus.evaluate (lib/dataset/shelf.py:255-330) on the device, accumulated over calls: ONE launch
 * of one workgroup (every counter has one writer), same inputs and participation rule as mvg_eval_match, J == 14.
 *   For every element b in order and every actor slot a < min(num_person[b], actors) with some joints_3d_vis[b, a, :] != 0: the
 *   participating row of smallest mean joint distance over all 14 joints (first minimum, NaN ordered as +inf); state[5] += (that
 *   mean < recall_threshold), state[1] += 1; the nine limb tests (e_start + e_end) / 2 <= alpha * length and the hip-centre / head
 *   test -> correct[a], total[a] (+= 10), bone_correct[a, 0..9] (int64, `actors` rows).  An element with such an actor and no
 *   participating row is not scored further and records state[6] = 1 + state[2] + b if state[6] is still 0.  state[2] += B,
 *   state[4] += the participating rows.
 * MVG_E_BADARG, and nothing launched, for shapes mvg_eval_match rejects, J != 14, actors < 1 or > MVG_EVAL_MAX_G, alpha < 0 or NaN,
 * a NaN recall_threshold, a NULL pointer other than count, a counter or state pointer that is not 8-byte aligned. */
int mvg_eval_pcp(const float* dets, const int* count, const float* joints_3d, const float* joints_3d_vis, const int* num_person, int B,
                 int R, int J, int Gmax, int actors, double recall_threshold, double alpha, int64_t* correct, int64_t* total,
                 int64_t* bone_correct, int64_t* state, void* stream);

/* ---- person identities across frames behind the NMS (csrc/track.hip) --------------------------------------------------------- */
#define MVG_LAP_MAX_N 64              /* rows and columns of one assignment problem: one wavefront, a lane per column          */
#define MVG_LAP_BIG 1e15              /* an entry that is NaN or above this is taken as this                                   */
#define MVG_TRACK_MAX_D 64            /* detections per stream and frame that take part                                        */
#define MVG_TRACK_MAX_T 64            /* track slots per stream                                                                */
#define MVG_TRACK_MAX_J 32
#define MVG_TRACK_MAX_R 16384         /* rows of dets per batch element                                                        */
#define MVG_TRACK_MAX_B 4096          /* batch elements (workgroups) of one call, of either function                           */
#define MVG_TRACK_STATE_WORDS 8       /* int64 state block: frames, matches, births, deaths, overflow, dropped, active,
                                       * reserved (the arrival counter of a call's workgroups; 0 between calls)                */

/* Minimum-cost assignment of B independent problems in ONE launch, one workgroup of one wavefront per problem, no host
 * involvement, bit-reproducible.  cost (B, N, M) fp64; n, m (B) int32 live sizes (clamped to [0, N] / [0, M]) or NULL = N, M.
 *   s = max(n, m); S[i, j] = cost[i, j] for i < n and j < m, 0.0 elsewhere (s x s); an entry that is NaN or > MVG_LAP_BIG is taken
 *   as MVG_LAP_BIG.  Shortest-augmenting-path Hungarian algorithm with potentials u (rows), v (columns), all 0 at the start, rows
 *   inserted in order 0 .. s-1.  The search of row i starts at a virtual column whose row is i, with minv[j] = +inf,
 *   way[j] = virtual, no column used; one step, with j0 the current column and i0 its row:
 *     1. j0 is marked used;
 *     2. for every unused column j: cur = (S[i0, j] - u[i0]) - v[j]; if cur < minv[j]: minv[j] = cur, way[j] = j0;
 *     3. j1 = the unused column of smallest minv, the LOWEST column among equal values, a NaN minv ordered as +inf (so without a
 *        finite minimum it is the lowest unused column); delta = minv[j1];
 *     4. u += delta for the rows of the used columns (row i of the virtual column included), v -= delta for the used columns,
 *        minv -= delta for the unused columns; j0 = j1.
 *   The search ends when j0 has no row; the path is then flipped along way[] back to the virtual column.  A search is a counted
 *   loop of at most s steps (step k uses a k-th column and at most i < s columns have a row): no input can make it spin.
 *   fp64 throughout, every operation rounded on its own.
 * Outputs: col_of_row (B, N) int32: the column of row r, -1 for r >= n and for a row assigned to a padding column (j >= m);
 * total (B) fp64: the sum of cost[r, col_of_row[r]] AS GIVEN (not clamped) over the assigned rows, added in row order.
 * MVG_E_BADARG, and nothing launched, for N or M < 1 or > MVG_LAP_MAX_N, B < 1 or > MVG_TRACK_MAX_B, a NULL cost / col_of_row /
 * total, a cost or total pointer that is not 8-byte aligned. */
int mvg_linear_assignment(const double* cost, const int* n, const int* m, int B, int N, int M, int* col_of_row, double* total,
                          void* stream);

/* One frame of the pose tracker for B independent streams in ONE launch (one workgroup per stream), fixed shapes, nothing read
 * back, integer atomics on the state block only, bit-reproducible; can be captured in a HIP graph behind mvg_pose_nms.
 *   dets (B, R, J, 5) fp32 rows [x, y, z, flag, score] and count (B, 2) int32 or NULL as mvg_pose_nms leaves them: row i of
 *   element b is a detection iff dets[b, i, 0, 3] >= 0 and (count == NULL or i < count[b, 0]).  Detections are taken in row order
 *   (the NMS keep order); the first MVG_TRACK_MAX_D take part, the others get id -1 and are counted in `dropped`.
 *   Track state, owned by the caller: id (B, T) int32 (-1 = free slot), hits, misses (B, T) int32, born (B, T) int64 (the frame
 *   number), score (B, T) fp32, pose (B, T, J, 3) fp32, next_id (B) int32, state (MVG_TRACK_STATE_WORDS) int64.
 *   Per element: (1) the active tracks are the slots with id >= 0, in slot order.  (2) c[t, d] = (sum over joints in order of
 *   sqrt((dx*dx + dy*dy) + dz*dz)) / J in fp64 from the fp32 inputs, correctly rounded sqrt (with the caveat of mvg_pose_nms:
 *   dy*dy and dz*dz are fused into their sums; mvg_track_eval rounds every product on its own).  (3) c'[t, d] = c[t, d] if
 *   c[t, d] <= max_dist, else max_dist (also for NaN).  (4) the solver of mvg_linear_assignment on c', active tracks as rows,
 *   detections as columns: every non-match pays max_dist through the zero padding, the matching is the global optimum.  (5) an
 *   assigned pair is a match iff the ungated c[t, d] <= max_dist.  (6) a matched track takes the detection's pose (bit for bit)
 *   and score (dets[b, row, 0, 4]), misses = 0, hits += 1.  (7) an unmatched track: misses += 1; if misses > max_misses the slot is
 *   freed (id = -1) and `deaths` counts it.  (8) the unmatched detections, in detection order, each open a track in the lowest
 *   free slot (slots freed in (7) included): id = next_id[b]++, hits = 1, misses = 0, born = state[0] as the call found it, pose
 *   and score of the detection; without a free slot the detection gets no track and `overflow` counts it.
 *   Outputs, every element written: slots (B, R) int32 = the slot of the row's track, -1 for a row that is no detection or has no
 *   track; ids (B, R) int32 = the track's id once its hits >= min_hits, else -1.
 *   State: matches, births, deaths, overflow, dropped += the element's counts, active += births - deaths (the live tracks, given
 *   that state and id were reset together); frames += 1 per CALL, by the last workgroup to arrive.
 * MVG_E_BADARG, and nothing launched, for B, R, J or T < 1 or above their MVG_TRACK_MAX_*, max_dist < 0, NaN or > MVG_LAP_BIG,
 * max_misses or min_hits < 0, a NULL pointer other than count, a born or state pointer that is not 8-byte aligned. */
int mvg_track_update(const float* dets, const int* count, int B, int R, int J, int T, int* id, int* hits, int* misses, int64_t* born,
                     float* score, float* pose, int* next_id, int64_t* state, double max_dist, int max_misses, int min_hits,
                     int* ids, int* slots, void* stream);

/* Constant-velocity motion model of the tracker: two launches AROUND an unchanged mvg_track_update (predict, update, correct), one
 * workgroup per stream each, fixed shapes, nothing read back, no atomics, every element with one writer: bit-reproducible, and
 * capturable in a HIP graph with the update.  Motion state, owned by the caller: mean (B, T, J, 2, 3) fp64 = position xyz and
 * velocity xyz per joint, var (B, T, 3) fp64 = pxx, pxv, pvv, ONE 2 x 2 covariance per track (the same noise on every joint and
 * axis: the covariance follows the track's hit / miss history, not the data).  fp64, every operation rounded on its own, in the
 * order written; (float) rounds to nearest even.
 *
 * mvg_track_predict, before the update: for every slot with id >= 0 (free slots are not touched), with dt2 = dt*dt, dt3 = dt2*dt,
 * dt4 = dt2*dt2, qxx = (q*dt4)/4, qxv = (q*dt3)/2, qvv = q*dt2:
 *   per joint and axis: x = x + v*dt; pose = (float) x;
 *   pxx' = ((pxx + (2*dt)*pxv) + dt2*pvv) + qxx;  pxv' = (pxv + dt*pvv) + qxv;  pvv' = pvv + qvv   (old values on the right).
 * The update then associates against the predicted poses; a track it does not match keeps its prediction.
 * MVG_E_BADARG, and nothing launched, for B, T or J < 1 or above their MVG_TRACK_MAX_*, a NULL pointer, a mean or var pointer that
 * is not 8-byte aligned, dt not finite or <= 0, q < 0, NaN or > MVG_LAP_BIG. */
int mvg_track_predict(int B, int T, int J, const int* id, float* pose, double* mean, double* var, double dt, double q, void* stream);

/* mvg_track_correct, after the update, every slot by its state as the update left it (id, hits, misses, slots are read only):
 *   free (id < 0): mean and var of the slot = 0.
 *   missed (id >= 0, misses > 0): nothing changes.
 *   born in this call (id >= 0, misses == 0, hits == 1; also a slot freed and reopened by the same update):
 *     x = (double) pose, v = 0, var = (r, 0, v0).
 *   matched (id >= 0, misses == 0, hits > 1): pose holds the detection z.  s = pxx + r; kx = pxx/s; kv = pxv/s; per joint and axis
 *     e = z - x; x = x + kx*e; v = v + kv*e; pose = (float) x; then pvv' = pvv - kv*pxv; pxv' = (1 - kx)*pxv; pxx' = (1 - kx)*pxx
 *     (old values on the right).
 *   Then for every row of slots (B, R): row_pose (B, R, J, 3) fp32 = pose of the row's slot, zeros where slots < 0: the filtered
 *   pose of every kept detection.
 * MVG_E_BADARG, and nothing launched, for B, R, T or J < 1 or above their MVG_TRACK_MAX_*, a NULL pointer, a mean or var pointer
 * that is not 8-byte aligned, r <= 0, v0 < 0, or either NaN or > MVG_LAP_BIG. */
int mvg_track_correct(int B, int R, int T, int J, const int* id, const int* hits, const int* misses, const int* slots, float* pose,
                      double* mean, double* var, double r, double v0, float* row_pose, void* stream);

#define MVG_TRACK_EVAL_MAX_P 64       /* identities per stream: the rows of the remaining-pairs solve and of the overlap table  */
#define MVG_TRACK_EVAL_MAX_K 4096     /* columns of the overlap table: track ids below this are counted                        */
#define MVG_TRACK_EVAL_WORDS 13       /* int64 counters per stream: frames, gt, hyp, matches, misses, false_pos, switches, kept,
                                       * dropped, unreported, bad_id, id_overflow, reserved (always 0)                          */

/* CLEAR-MOT counts and the identity overlap table of one frame of the tracker's output against ground truth, for B independent
 * streams in ONE launch (one workgroup per stream) behind mvg_track_update (or mvg_track_correct), fixed shapes, nothing read
 * back, NO atomics: every element of the state has one writer, the stream's own workgroup, so the bits cannot depend on the order
 * of the workgroups; capturable in a HIP graph.
 *   dets (B, R, J, 5) fp32 and count (B, 2) int32 or NULL as mvg_pose_nms leaves them; ids (B, R) int32, the tracker's per-row
 *   ids; row_pose (B, R, J, 3) fp32 or NULL: when given, a hypothesis' pose is taken from here (the motion model's filtered
 *   poses) instead of dets.  Ground truth in the evaluator's layout: joints_3d (B, G, J, 3) fp32, joints_3d_vis (B, G, J) fp32
 *   (visible when > 0), num_person (B) int32; person_id (B, G) int32 or NULL (the identity of person slot g is g).
 *   State, owned by the caller, P identities per stream (G <= P <= MVG_TRACK_EVAL_MAX_P), K columns: last_track (B, P) int32
 *   (-1 at the start), counters (B, MVG_TRACK_EVAL_WORDS) int64, dist_sum (B) fp64, seen, covered (B, P) int64, overlap (B, P, K)
 *   int32, all 0 at the start.
 * Per stream b:
 *   1. Frame skipping.  num_person[b] < 0: the frame has no annotation, nothing is counted or changed.  num_person[b] == 0 is an
 *      annotated empty frame (every hypothesis is a false positive).
 *   2. Hypotheses: the rows i < count[b, 0] (clamped to [0, R]; all R rows when count is NULL) with dets[b, i, 0, 3] >= 0 AND
 *      ids[b, i] >= 0, in row order, the first MVG_TRACK_MAX_D; later ones are counted in `dropped`.  Detection rows (flag >= 0,
 *      in front of the count) with ids < 0 are no hypotheses and are counted in `unreported`.  The ids of a stream's hypotheses
 *      are expected to be distinct, as mvg_track_update's are; with equal ids one of the concurrent += 1 on the same overlap
 *      entry in 9 may be lost, nothing else is affected.
 *   3. Persons: the slots g < min(num_person[b], G) with at least one visible joint, in slot order, identity p = person_id[b, g]
 *      (or g).  A person whose p is outside [0, P), or equal to the p of a person in a lower slot, is counted in `bad_id` and
 *      ignored.
 *   4. d[person, hypothesis] = (sum over the person's VISIBLE joints in joint order of sqrt((dx*dx + dy*dy) + dz*dz)) / (the
 *      number of visible joints), fp64 from the fp32 inputs, every operation rounded on its own, correctly rounded sqrt.  A NaN
 *      distance is no match (d <= dist_thr is false).
 *   5. Kept correspondences, persons in slot order: with h the first hypothesis in row order whose id is last_track[b, p]
 *      (last_track >= 0): if no earlier person has kept h and d[person, h] <= dist_thr the pair is matched, whatever the optimum
 *      of 6 would pair, and counted in `kept`.
 *   6. The remaining persons (slot order) x the remaining hypotheses (row order): the solver of mvg_linear_assignment on
 *      c' = d if d <= dist_thr else dist_thr (also for NaN); an assigned pair is a match iff its ungated d <= dist_thr.
 *   7. For each person in slot order: seen[b, p] += 1.  Matched with the hypothesis of id t: matches += 1, dist_sum[b] =
 *      dist_sum[b] + d (one add per match, in this order), covered[b, p] += 1; if last_track[b, p] >= 0 and != t: switches += 1;
 *      last_track[b, p] = t.  Not matched: misses += 1, last_track stays (a person who comes back under another id is one switch).
 *   8. false_pos += the unmatched hypotheses; gt += the persons, hyp += the hypotheses, frames += 1.
 *   9. For every (person, hypothesis) pair with d <= dist_thr, matched or not, t the hypothesis' id: overlap[b, p, t] += 1 when
 *      t < K, otherwise id_overflow += 1.
 * MVG_E_BADARG, and nothing launched, for B, R or J < 1 or above their MVG_TRACK_MAX_*, G < 1, P < G or > MVG_TRACK_EVAL_MAX_P,
 * K < 1 or > MVG_TRACK_EVAL_MAX_K, dist_thr < 0, NaN or > MVG_LAP_BIG, a NULL pointer other than count, row_pose and person_id, a
 * counters, dist_sum, seen or covered pointer that is not 8-byte aligned. */
int mvg_track_eval(const float* dets, const int* count, const int* ids, const float* row_pose, const float* joints_3d,
                   const float* joints_3d_vis, const int* num_person, const int* person_id, int B, int R, int J, int G, int P, int K,
                   double dist_thr, int* last_track, int64_t* counters, double* dist_sum, int64_t* seen, int64_t* covered,
                   int* overlap, void* stream);

/* ---- structural triangulation: fixed bone lengths (csrc/structural.hip) ------------------------------------------------------- */
#define MVG_ST_MAX_J 17               /* joints of a tree: the reduced system has 3 (J - 1) <= 48 rows, a lane each             */
#define MVG_ST_MAX_V 32
#define MVG_ST_MAX_STEPS 8
#define MVG_ST_LS 0                   /* the unconstrained least squares in bone coordinates                                   */
#define MVG_ST_ST 1                   /* n_steps constrained steps towards the given bone lengths                              */

/* A person's J joints from their 2D observations in V views under fixed bone lengths (lib/structural/structural_triangulation.py:
 * Pose3D_inference with method 'ST' / 'LS'), ONE launch, one wavefront per person, fixed shapes, nothing read back, no atomics,
 * every element with one writer: bit-reproducible, a person's result does not depend on the others, capturable in a HIP graph.
 *   ud (B, V, NQ*J, 2) undistorted original-image px, conf (B, V, NQ*J) weights or NULL (= 1 / V, in fp64), Pm (B, V, 3, 4) =
 *   [KR | t], all fp32, the layout of mvg_dlt_forward.  parent: J HOST ints, by value in the launch arguments: parent[0] = -1 (the
 *   root), every other joint reaches joint 0 along parent[] (any index order).  Bone k (k = 1 .. J-1) ends at joint k; anc(i) =
 *   the bones on the path root -> i.  bone_len fp32: (J-1) shared, or (B, P, J-1) with bone_len_per_person != 0; entry k-1 is
 *   bone k; not read (may be NULL) for MVG_ST_LS.
 *   Persons, P per batch element:  rows == NULL (dense; P must equal NQ): person (b, p) is query p if valid == NULL or
 *   valid[b, p] != 0 (valid (B, NQ) uint8).  rows != NULL: rows (B, P) int32 with row stride rows_ld >= P, count (B, 2) int32 or
 *   NULL as mvg_pose_nms writes keep and count: person (b, p) is query rows[b, p] for p < min(max(count[b, 0], 0), P) (P without
 *   count) and 0 <= rows[b, p] < NQ; valid must be NULL.
 * Arithmetic: fp64 from the fp32 inputs, every product and sum rounded on its own, division and sqrt correctly rounded; "sum" =
 * an accumulation from +0.0 in ascending index order by one lane.  n = 3 (J - 1), K = J - 1.
 *   1. Per joint i, views ascending: g0 = r0 - u r2, g1 = r1 - w r2 (r = the rows of KR), h0 = t0 - u t2, h1 = t1 - w t2,
 *      c2 = 2 c;  D_i[a][b] += c2 (g0[a] g0[b] + g1[a] g1[b]);  m_i[a] -= c2 (g0[a] h0 + g1[a] h1)   (KR^T M KR = g0 g0^T + g1 g1^T
 *      for the reference's M = [[1, 0, -u], [0, 1, -w], [-u, -w, u^2 + w^2]]).
 *   2. T = sum_i D_i, mu = sum_i m_i;  C_k = sum_{i: k in anc(i)} D_i, cm_k likewise from m_i (i ascending).  Tinv = T^-1 by the
 *      factorisation below.  W_k = Tinv C_k, tm = Tinv mu (sums over the inner index).  For c <= r, with r = 3 (k-1) + a,
 *      c = 3 (l-1) + bb:  A[r][c] = base - sum_t C_k[a][t] W_l[t][bb],  base = C_l[a][bb] if k in anc(l), else C_k[a][bb] if l in
 *      anc(k), else 0.  beta[r] = cm_k[a] - sum_t C_k[a][t] tm[t].
 *   3. Inv = A^-1 by the factorisation below;  b[r] = sum_c Inv[r][c] beta[c].  MVG_ST_LS goes to 5.
 *   4. For s = 0 .. n_steps-1:  start_k = sqrt((b0 b0 + b1 b1) + b2 b2) of bone k's three entries;
 *      target_k = (start_k (n_steps-s-1) + L_k) / (n_steps-s);  rhs_k = (start_k start_k - target_k target_k) / 4;
 *      S[k][l] = sum_a b_k[a] (sum_c Inv[3k+a][3l+c] b_l[c]) for l <= k;  S = L L^T as below;  y_i = (rhs_i - sum_{k<i} L[i][k] y_k)
 *      / L[i][i] (i ascending), lambda_i = (y_i - sum_{k>i ascending} L[k][i] lambda_k) / L[i][i] (i descending);  for c <= r:
 *      Inv'[r][c] = Inv[r][c] - sum_j (Inv[r][j] (2 lambda_{j/3})) Inv[j][c], written to both triangles;  b = Inv' beta as in 3.
 *   5. x0[a] = sum_t Tinv[a][t] (mu[t] - sum_j Cflat[t][j] b[j]) with Cflat[t][3 (k-1) + c] = C_k[t][c];  x_i = x0 + the b_k of
 *      k in anc(i), k ascending;  X = (float) x, round to nearest even.
 *   Factorisation of a symmetric M (its lower triangle): Cholesky column by column, j ascending: s_i = M[i][j] -
 *   sum_{k<j ascending} L[i][k] L[j][k] for i >= j; the pivot s_j must be > 0 (a NaN is not); L[j][j] = sqrt(s_j), L[i][j] =
 *   s_i / L[j][j].  Inverse: Y = L^-1 by Y[i][c] = ((i == c ? 1 : 0) - sum_{k=c}^{i-1} L[i][k] Y[k][c]) / L[i][i] for i >= c, then
 *   M^-1[r][c] = sum_{k=r}^{n-1} Y[k][r] Y[k][c] for c <= r, written to both triangles.
 * Outputs, every element written by every call: X (B, P, J, 3) fp32 and status (B, P) int32:
 *    0  solved;   1  a pivot of T or A was not > 0 (degenerate or non-finite input): X = 0;
 *    2  a pivot of S was not > 0 at some step: X from the b of the last completed step (the LS solution at the first);
 *   -1  not computed (valid == 0, a row at or behind the count, a row index outside [0, NQ)): X = 0.
 * Every loop is counted: no input can make the kernel spin or fault.
 * MVG_E_BADARG, and nothing launched, for J < 2 or > MVG_ST_MAX_J, V < 1 or > MVG_ST_MAX_V, n_steps < 1 or > MVG_ST_MAX_STEPS, an
 * unknown method, B, NQ or P < 1, a parent table that is no tree rooted at joint 0, a NULL ud / Pm / X / status / parent, a NULL
 * bone_len with MVG_ST_ST, rows with valid or rows_ld < P, no rows with count or P != NQ. */
int mvg_structural_triangulate(const float* ud, const float* conf, const float* Pm, const uint8_t* valid, const int* rows, int rows_ld,
                               const int* count, const int* parent, const float* bone_len, int bone_len_per_person, int method,
                               int n_steps, float* X, int* status, int V, int B, int NQ, int P, int J, void* stream);

/* ---- per-track bone lengths from the tracker's history (csrc/bones.hip) ------------------------------------------------------- */
#define MVG_BONES_MAX_W 32            /* samples a slot's ring holds                                                           */

/* The bone lengths of every tracked person, estimated over the frames the tracker has followed them, as the per-person bone_len
 * of mvg_structural_triangulate: ONE launch per frame behind mvg_track_update (and mvg_track_correct), in front of
 * mvg_structural_triangulate, one workgroup per stream, fixed shapes, nothing read back, NO atomics, every element with one
 * writer, every loop counted: bit-reproducible, a stream's result does not depend on the others, capturable in a HIP graph.
 *   dets (B, R, J, 5) fp32 and count (B, 2) int32 or NULL as mvg_pose_nms leaves them; slots (B, R) and id (B, T) int32 as
 *   mvg_track_update leaves them: both are read only, nothing of the tracker's is written.  parent: J HOST ints, the tree of
 *   mvg_structural_triangulate (parent[0] = -1, bone k = 1 .. J-1 ends at joint k), by value in the launch arguments.
 *   State, owned by the caller: owner (B, T) int32, -1 at the start: the track id whose history the slot holds; seen (B, T) int32,
 *   0 at the start; hist (B, T, W, J-1) fp32, the ring of the slot's last W samples; length (B, T, J-1) fp32, 0 at the start.
 * Per stream b, in this order:
 *   1. Ownership.  For every slot t with id[b, t] != owner[b, t]: owner = id, seen = 0, length[b, t, :] = 0 (a freed slot, id -1,
 *      and a slot freed and reopened by the same update alike: a stream's ids never repeat).
 *   2. Sample.  Row i is a detection iff i < count[b, 0] (clamped to [0, R]; every row without count) and dets[b, i, 0, 3] >= 0.
 *      For every detection row with s = slots[b, i] in [0, T):  len[k-1] = (float) sqrt((dx*dx + dy*dy) + dz*dz) of joint k and
 *      joint parent[k], k = 1 .. J-1, in fp64 from the RAW fp32 dets row (not the tracker's filtered pose), every product and sum
 *      rounded on its own, correctly rounded sqrt, one rounding to fp32.  If all J-1 values are finite: hist[b, s, seen mod W, :]
 *      = len, then seen = min(seen + 1, 2^30).  If several rows name the same slot (mvg_track_update never does that) the lowest
 *      row is the sample and the others are none.
 *   3. Estimate.  Only for the slots that took a sample in this call, with n = min(seen, W): length[b, s, k] = the median of
 *      hist[b, s, 0 .. n-1, k]: the middle value for n odd, (float)(((double) lo + (double) hi) * 0.5) of the two middle values
 *      for n even.  The values are selected by rank, rank = the number of smaller samples plus the number of equal samples at a
 *      lower index: ties cannot change the value.
 *   4. Rows, every element written by every call: row_length (B, R, J-1) fp32 and row_source (B, R) int32:
 *      -1  the row is no detection: zeros;
 *       0  a detection whose slot is in [0, T) with seen >= min_frames (as 2 left it): length of the slot;
 *       1  otherwise, with fallback (J-1 fp32) given: fallback;
 *       2  otherwise: the row's own len of 2 as computed, finite or not (the solver's status says what it made of them).
 *      Detections behind the first MVG_TRACK_MAX_D have no slot and take 1 or 2.
 * MVG_E_BADARG, and nothing launched, for B, R or T < 1 or above their MVG_TRACK_MAX_*, J < 2 or > MVG_ST_MAX_J, W < 1 or >
 * MVG_BONES_MAX_W, min_frames < 1, a parent table that is no tree rooted at joint 0, a NULL pointer other than count and
 * fallback. */
int mvg_track_bones(const float* dets, const int* count, const int* slots, const int* id, const int* parent, int B, int R, int J,
                    int T, int W, int min_frames, const float* fallback, int* owner, int* seen, float* hist, float* length,
                    float* row_length, int* row_source, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVG_DECODER_H */
