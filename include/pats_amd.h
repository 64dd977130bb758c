/*
 * pats_amd.h - C ABI of libpats_amd.so: the MI355X (gfx950) implementation of the PATS
 * patch-area optimal-transport hot path.
 *
 * Every entry point takes plain DEVICE pointers (fp32 / int64 / uint8, contiguous, row-major,
 * layouts exactly as the reference's tensors) plus sizes and a HIP stream; no torch types.  All
 * launches are asynchronous on `stream` (NULL = the default stream); nothing synchronises the
 * device unless stated.  Return value: PATS_OK or a PATS_ERR_* code, message in pats_last_error().
 * Inputs are never modified unless the name says `_inplace`.  Thread-safe (stateless).
 *
 * Citations are paths relative to the reference repository (zju3dv/pats).
 */
#ifndef PATS_AMD_H
#define PATS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pats_stream_t; /* hipStream_t */

enum {
    PATS_OK = 0,
    PATS_ERR_INVALID = 1,     /* bad shape / null pointer / workspace too small  (reference: TORCH_CHECK -> RuntimeError) */
    PATS_ERR_UNSUPPORTED = 2, /* shape outside what the kernels cover */
    PATS_ERR_LAUNCH = 3,      /* hip launch / runtime failure */
    PATS_ERR_NO_DEVICE = 4
};

/* Sinkhorn arithmetic.  LOG = max-subtracted log-sum-exp sweeps exactly as
 * models/modules.py:137-143.  KERNEL = the same fixed-point iteration carried in the linear
 * domain on K = exp(Z + u1 + v1) after one LOG warm-up sweep (row/col normalisation by
 * matrix-vector products, duals folded back into log space at the end), with an in-kernel guard
 * that re-runs a problem in LOG when its scaling vectors leave the safe fp32 range.  AUTO = KERNEL
 * where implemented, LOG otherwise. */
enum { PATS_SINKHORN_AUTO = 0, PATS_SINKHORN_LOG = 1, PATS_SINKHORN_KERNEL = 2 };

const char* pats_version(void);
/* The ABI this header describes.  It is bumped whenever an exported function changes its argument list (round 2 added
 * `row_nomatch` to pats_iterative_expand_f32 under the same symbol: a caller built against the older header would pass
 * its stream where the new pointer goes).  A C consumer checks `pats_abi_version() == PATS_ABI_VERSION` once after
 * loading the library; pats_amd/_lib.py does.  New arguments now come with new entry points instead. */
#define PATS_ABI_VERSION 8
int pats_abi_version(void);
const char* pats_last_error(void);
/* number of HIP devices visible (0 on a CPU-only box; never fails) */
int pats_device_count(void);
/* process-wide default for PATS_SINKHORN_AUTO (returns the previous value) */
int pats_set_sinkhorn_mode(int mode);
/* Fine level of pats_cost_ot_f32 / pats_cost_ot_flags_f32 (variant 2, 145 x 145): 0 (default) = the MFMA cost kernel, then the
 * register-block Sinkhorn kernel; 1 = ONE kernel that builds the score tile, turns it into the register blocks through LDS
 * and solves - the scores never reach HBM (second_layer.py:100-105 in one launch).  Same bits either way
 * (tests/test_gpu_parity.py); measured 5.69 against 5.62 ms per 20 224 problems.  Returns the
 * previous setting; PATS_FINE_FUSED=1 in the environment sets the initial one. */
int pats_set_fine_fused(int on);

/* Which kernel takes the fp32 third-level gather on NCHW maps (pats_third_descriptors_f32, _counted_f32 and the fp32 NCHW route of
 * pats_third_descriptors_typed): 0 (default) the point-tiled third_desc_kernel, 1 the per-point third_desc_point_kernel.  Same
 * bits either way.  Returns the previous setting; any other argument leaves it unchanged.  Process-wide. */
int pats_set_third_gather(int mode);

/* Number of problems (on the current device, since the last reset) whose linear-domain solve left the
 * guard band and was re-solved with log-sum-exp sweeps.  Results are the same either way; a high rate
 * only costs time.  Synchronises the whole device (hipDeviceSynchronize) before the read and after the
 * reset, so launches on any stream are counted and none races with the reset.  No reference counterpart. */
int pats_sinkhorn_fallbacks(int64_t* count, int reset);

/* Of those, the 145 x 145 problems whose STABILISED linear re-solve (sinkhorn_rc_kernel, linear == 2) failed its final guard as
 * well and were solved by the log-sum-exp sweeps behind it, in the same launch: problems with non-finite scores, or whose
 * scalings run away within a single sweep.  The plan is the same either way, so nothing else shows that the stabilised form
 * stopped working.  The count also covers the third level's 65 x 65 stabilised re-solve (third_fused3_stab_kernel): a problem it
 * leaves to third_fused_kernel's log-sum-exp sweeps because a scaling left (0, 3e38] within one sweep.
 * Same synchronisation and reset as pats_sinkhorn_fallbacks, a counter of its own.  No reference counterpart. */
int pats_sinkhorn_tail_solves(int64_t* count, int reset);

/* ---- a1-a3: cost build -------------------------------------------------------------------
 * out[b,i,j] = 0.1f * ( (sum_d d0[b,d,i] * d1[b,d,j]) / sqrtf(D) )
 * replaces  scores = einsum('bdn,bdm->bnm', mdesc0, mdesc1) / D**.5 ; 0.1 * scores
 *           models/first_layer.py:110-111,114  second_layer.py:100-101,104  third_layer.py:156-158
 * d0 [batch,D,n], d1 [batch,D,m] (channel-major), out [batch,n,m].  fp32 in, fp32 out; the contraction splits every
 * operand into an fp16 hi + lo pair (exact products on the fp16 matrix pipe, fp32 accumulation: on operands of magnitude
 * 0.004 .. 1023 at least as close to float64 as an fp32 fma chain; an operand below 0.004 has a subnormal lo half, which the
 * matrix pipe flushes, and is carried with an absolute error <= 2^-20, i.e. <= 1e-6 |y| per product) and redoes a tile with the fp32 MFMA when an operand exceeds +-1023. */
int pats_cost_f32(const float* d0, const float* d1, int64_t batch, int D, int n, int m, float* out,
                  pats_stream_t stream);

/* ---- a6: log_sinkhorn_iterations(Z, log_mu, log_nu, iters)  models/modules.py:137-143 ------
 * Z [batch,M,N], log_mu [batch,M], log_nu [batch,N] -> out [batch,M,N] = Z + u + v.
 * workspace: pats_sinkhorn_workspace_bytes(batch, M, N) bytes of device memory (may be NULL if
 * that returns 0). */
size_t pats_sinkhorn_workspace_bytes(int64_t batch, int M, int N);
int pats_sinkhorn_f32(const float* Z, int64_t batch, int M, int N, const float* log_mu,
                      const float* log_nu, int iters, float* out, void* workspace,
                      size_t workspace_bytes, pats_stream_t stream);

/* ---- a4: log_optimal_transport(scores, alpha, ns, iters)  models/modules.py:145-162 --------
 * scores [batch,m,n]; alpha: DEVICE pointer to one float (the reference's 0-d `bin_score.abs()`);
 * ns [batch,n] target areas (the reference's [b,1,n]) -> Z [batch,m+1,n+1] log-plan with dustbin
 * row/col, already `- norm`.  workspace: pats_ot_workspace_bytes(batch, m+1, n+1). */
size_t pats_ot_workspace_bytes(int64_t batch, int M, int N);
int pats_log_optimal_transport_f32(const float* scores, int64_t batch, int m, int n,
                                   const float* alpha, const float* ns, int iters, float* Z,
                                   void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ---- a5: log_optimal_transport2(scores, one, ns, iters)  models/modules.py:165-182 ---------
 * scores [batch,m,n] whose last row/col are already the dustbin; one: DEVICE pointer to one float
 * or NULL (= 1.0f); ns [batch,n-1] -> Z [batch,m,n].  bias_k > 0 additionally applies the
 * caller's  Z[:,:,-1] += log(k); Z[:,-1,:] += log(k)  (second_layer.py:107-112); 0 = none.
 * workspace: pats_ot2_workspace_bytes(batch, m, n) - 0 for 65 x 65, one guard flag per problem for
 * 145 x 145 (the resident kernels), pats_ot_workspace_bytes otherwise. */
size_t pats_ot2_workspace_bytes(int64_t batch, int m, int n);
/* the same plus est_position's if_nomatching2 = (Z.max(1).indices == m-1) for the first n-1 columns
 * (second_layer.py:243,248; first index wins ties): col_nomatch [batch,n-1] uint8, written by the 145 x 145
 * kernel's own epilogue (other shapes: one extra pass over Z).  Row flags come from pats_iterative_expand_f32. */
int pats_log_optimal_transport2_flags_f32(const float* scores, int64_t batch, int m, int n,
                                          const float* one, const float* ns, int iters, float bias_k,
                                          float* Z, uint8_t* col_nomatch, void* workspace,
                                          size_t workspace_bytes, pats_stream_t stream);
int pats_log_optimal_transport2_f32(const float* scores, int64_t batch, int m, int n,
                                    const float* one, const float* ns, int iters, float bias_k,
                                    float* Z, void* workspace, size_t workspace_bytes,
                                    pats_stream_t stream);

/* ---- a1-a3 + a4/a5 fused: descriptors -> log-plan, no score matrix round trip ---------------
 * variant 1 = log_optimal_transport (Z [batch,n+1,m+1], ns [batch,m]);
 * variant 2 = log_optimal_transport2 (Z [batch,n,m], ns [batch,m-1]).
 * scalar = alpha (variant 1) or one (variant 2), device pointer (NULL = 0 / 1). */
int pats_cost_ot_f32(const float* d0, const float* d1, int64_t batch, int D, int n, int m,
                     int variant, const float* scalar, const float* ns, int iters, float bias_k,
                     float* Z, void* workspace, size_t workspace_bytes, pats_stream_t stream);
size_t pats_cost_ot_workspace_bytes(int64_t batch, int D, int n, int m, int variant);
/* variant 2 with the column flags of pats_log_optimal_transport2_flags_f32 (same workspace). */
int pats_cost_ot_flags_f32(const float* d0, const float* d1, int64_t batch, int D, int n, int m,
                           int variant, const float* scalar, const float* ns, int iters, float bias_k,
                           float* Z, uint8_t* col_nomatch, void* workspace, size_t workspace_bytes,
                           pats_stream_t stream);

/* Measurement hook: `event` (a hipEvent_t, or NULL) is recorded once, by the next two-kernel pats_cost_ot*_f32 call of the calling
 * thread, between its cost-build launch and its Sinkhorn launch (bench.py times the two kernels inside its steps with it).  ABI 5. */
int pats_set_cost_ot_mid_event(void* event);

/* The fine level launched over a CAPACITY of batch_cap problems with the number in use on the device (throughput mode:
 * batch_dev = the row table's total, &chunk_base[Cmax] of pats_chunk_rows_device): workgroups of problems >= *batch_dev return
 * at once - no cost build, no solve, no log-domain redo; their rows of Z / col_nomatch are left untouched.  variant 2,
 * n = m = 145 only; everything else as pats_cost_ot_flags_f32 (workspace sized for batch_cap).  ABI 5. */
int pats_cost_ot_flags_counted_f32(const float* d0, const float* d1, int64_t batch_cap, const int64_t* batch_dev,
                                   int D, int n, int m, int variant, const float* scalar, const float* ns, int iters,
                                   float bias_k, float* Z, uint8_t* col_nomatch, void* workspace,
                                   size_t workspace_bytes, pats_stream_t stream);

/* ---- a7: post-OT reductions ----------------------------------------------------------------
 * colmass: out[b,j] = sqrtf(sum_{i<M-1} expf(Z[b,i,j]) + 1e-8f), j < N-1   first_layer.py:117-118
 * bias   : Z[:,:,-1] += logf(k); Z[:,-1,:] += logf(k) in place              second_layer.py:107-112
 * exp    : out = expf(Z)                                                    third_layer.py:159 */
int pats_colmass_sqrt_f32(const float* Z, int64_t batch, int M, int N, float* out,
                          pats_stream_t stream);
/* colmass plus est_position's if_nomatching2 = (scores.max(1).indices == M-1) in the same pass over the
 * columns (first_layer.py:163,167): col_nomatch [batch,N-1] uint8.  Either output may be NULL. */
int pats_colmass_flags_f32(const float* Z, int64_t batch, int M, int N, float* out, uint8_t* col_nomatch,
                           pats_stream_t stream);
int pats_dustbin_bias_inplace_f32(float* Z, int64_t batch, int M, int N, float k,
                                  pats_stream_t stream);
int pats_exp_f32(const float* Z, int64_t count, float* out, pats_stream_t stream);

/* ---- a8: scores.max(2).indices / scores.max(1).indices, first index wins ties ---------------
 * first_layer.py:162  second_layer.py:243.  row_arg [batch,M], col_arg [batch,N]; either NULL. */
int pats_argmax_f32(const float* Z, int64_t batch, int M, int N, int64_t* row_arg,
                    int64_t* col_arg, pats_stream_t stream);

/* ---- a9-a11: Iterative_expand_matrix + Compute_scaling  utils/utils.py:1179-1297,1321-1340 --
 * P [batch,M,N] = exp(Z) incl. dustbin row/col (or Z itself when input_is_log != 0: the kernel
 * exponentiates on load, saving the exp(Z) round trip of first_layer.py:174 / second_layer.py:255);
 * scalex, scaley [batch,N-1]; lim3 = limitation[3]; (h, w) = the TRUE grid the caller built
 * positions/ranges for (Compute_positions_and_ranges, utils.py:1527-1537).
 * outputs: whole_cost, core_cost, x_scale, y_scale [batch,M-1]; average_point [batch,M-1,2];
 * bound [batch,M-1,4] int64 (up,down,left,right).
 *
 * row_nomatch (optional, [batch,M-1] uint8): est_position's if_nomatching1 = (scores.max(2).indices == N-1)
 * (first_layer.py:162-164, second_layer.py:243-245) taken from the values as handed in - the row is in LDS
 * here anyway, so the separate argmax pass over the plan disappears. */
int pats_iterative_expand_f32(const float* P, int input_is_log, int64_t batch, int M, int N,
                              const float* scalex, const float* scaley, int lim3, int h, int w,
                              float lower_bound, int iter_num, float* whole_cost, float* core_cost,
                              float* average_point, float* x_scale, float* y_scale, int64_t* bound,
                              uint8_t* row_nomatch, pats_stream_t stream);

/* The same over a capacity of batch_cap problems, *batch_dev of them in use (device-side count); the outputs of the others are
 * left untouched.  ABI 5. */
int pats_iterative_expand_counted_f32(const float* P, int input_is_log, int64_t batch_cap, const int64_t* batch_dev,
                                      int M, int N, const float* scalex, const float* scaley, int lim3, int h, int w,
                                      float lower_bound, int iter_num, float* whole_cost, float* core_cost,
                                      float* average_point, float* x_scale, float* y_scale, int64_t* bound,
                                      uint8_t* row_nomatch, pats_stream_t stream);

/* ---- a12: split_patches(sum_cycle, height, width, max_once_used)  utils/utils.py:152-181 ----
 * HOST function on a host copy of the int32 cumsum (the reference syncs per comparison; here the
 * caller pays one D->H copy).  second/third: [height+1][2] int64.  Returns cycle_num (>= 1), or
 * a negative PATS_ERR code. */
int pats_split_patches(const int32_t* sum_cycle_host, int height, int width, int max_once_used,
                       int64_t* second_layer_set, int64_t* third_layer_set);
/* The same planner on the DEVICE for a batch of pairs (throughput mode: no host read at all):
 * sum_cycle [pairs, height*width] int32 device cumsums -> second/third [pairs, height+1, 2] int64
 * (unused rows zeroed) and cycle_num [pairs] int32, all device memory.  One thread per pair. */
int pats_split_patches_device(const int32_t* sum_cycle, int64_t pairs, int height, int width,
                              int max_once_used, int64_t* second_layer_set, int64_t* third_layer_set,
                              int32_t* cycle_num, pats_stream_t stream);

/* ---- a13: Compute_imgs bounds  utils/utils.py:1350-1382 ------------------------------------
 * x_scale, y_scale [Np]; average_point [Np,2]; if_nomatching [Np] uint8; grid (height,width).
 * -> bound5 [Np,5] int64, only the first *K rows valid (y0,y1,x0,x1,img*10000+patch) in patch
 *    order; K_out: DEVICE int64 count; x_scale_new, y_scale_new, average_new [Np,2]. */
int pats_compute_imgs_bounds_f32(const float* x_scale, const float* y_scale,
                                 const float* average_point, const uint8_t* if_nomatching, int Np,
                                 int height, int width, int img, int64_t* bound5, int64_t* K_out,
                                 float* x_scale_new, float* y_scale_new, float* average_new,
                                 pats_stream_t stream);

/* ---- a13: left crops = origin_extract on the 32-px padded left image  utils.py:1300-1318,1383
 * left [n_img,H,W,3] HWC fp32; bound5/K as produced above (row k: image bound5[k,4] / 10000, patch
 * bound5[k,4] % 10000, the reference's `sequence`, utils.py:1374-1377) -> out [K,96,96,3].  K is read on
 * the host side by the caller (max rows = K_cap). */
int pats_left_crops_f32(const float* left, int n_img, int H, int W, const int64_t* bound5, int64_t K,
                        int height, int width, float* out, pats_stream_t stream);

/* a13 for a BATCH of images without host-side counts (throughput mode).  x_scale, y_scale [n_img,Np],
 * average_point [n_img,Np,2], if_nomatching [n_img,Np] -> bound5 [n_img*Np,5] compacted in (image, patch)
 * order (sequence = img * 10000 + patch, utils.py:1374-1377), K_img [n_img] matches per image and
 * K_total [1] = valid rows of bound5 (DEVICE int64), x_scale_new, y_scale_new, average_new [n_img,Np,2].
 * The `_counted` gathers are launched over K_cap rows and skip rows >= *K_dev. */
int pats_compute_imgs_bounds_batch_f32(const float* x_scale, const float* y_scale, const float* average_point,
                                       const uint8_t* if_nomatching, int n_img, int Np, int height, int width,
                                       int64_t* bound5, int64_t* K_img, int64_t* K_total, float* x_scale_new,
                                       float* y_scale_new, float* average_new, pats_stream_t stream);
int pats_left_crops_counted_f32(const float* left, int n_img, int H, int W, const int64_t* bound5,
                                int64_t K_cap, const int64_t* K_dev, int height, int width, float* out,
                                pats_stream_t stream);

/* ---- a14: tensor_resize(input, bound)  setup/library.cpp:47-66 (module def :92-93) ----------
 * input [n_img,C,Hp,Wp] fp32; bound [K,5] int64 (y0,y1,x0,x1,seq), image = seq / 10000;
 * crop rows [y0,y1) x cols [x0,x1] -> bilinear align_corners=True -> out [K,C,96,96].
 * One launch, no host sync (the reference does 5 .item() syncs per crop).  status: optional DEVICE
 * int32 that is set non-zero if any crop is empty / out of range (torch raises there); the kernel
 * itself clamps reads so it is always memory-safe.  K == 0 is a no-op. */
int pats_tensor_resize_f32(const float* input, int n_img, int C, int Hp, int Wp,
                           const int64_t* bound, int64_t K, float* out, int32_t* status,
                           pats_stream_t stream);
/* same, fused with the zero padding of utils.py:1352 and the HWC->CHW permute: reads the
 * UNPADDED right image [n_img,H,W,3] (margin = 128) and writes [K,96,96,3] (the layout the caller
 * permutes to at utils.py:1385). */
int pats_tensor_resize_hwc_f32(const float* right, int n_img, int H, int W, int margin,
                               const int64_t* bound, int64_t K, float* out, int32_t* status,
                               pats_stream_t stream);
int pats_tensor_resize_hwc_counted_f32(const float* right, int n_img, int H, int W, int margin,
                                       const int64_t* bound, int64_t K_cap, const int64_t* K_dev, float* out,
                                       int32_t* status, pats_stream_t stream);

/* ---- a17 + a18: ThirdLayer.Compute_result + match label  models/third_layer.py:161-170,184-217
 * scores [P,65,65] = exp(Z) (or Z when input_is_log); scale_x, scale_y [P,64]; p_s, p_t [P,2]
 * int64 -> mkpts0_f, mkpts1_f [P,16,2]; whole_loss [P,16]; label [P*16,2]; if_matching1 [P,16]
 * uint8.  W = 8, T = 5 as in the reference. */
int pats_compute_result_f32(const float* scores, int input_is_log, int64_t P, const float* scale_x,
                            const float* scale_y, const int64_t* p_s, const int64_t* p_t,
                            int outdoor, float* mkpts0_f, float* mkpts1_f, float* whole_loss,
                            float* label, uint8_t* if_matching1, pats_stream_t stream);
/* the same with the 4 bytes of device workspace whole_loss needs (its cross-problem count, :215) handed in by the
 * caller: no allocation inside the call (pats_compute_result_f32 takes a stream-ordered one), capturable in a HIP graph */
int pats_compute_result_ws_f32(const float* scores, int input_is_log, int64_t P, const float* scale_x,
                               const float* scale_y, const int64_t* p_s, const int64_t* p_t,
                               int outdoor, float* mkpts0_f, float* mkpts1_f, float* whole_loss,
                               float* label, uint8_t* if_matching1, void* workspace, size_t workspace_bytes,
                               pats_stream_t stream);

/* ---- a15: fine-level descriptor sampling  models/second_layer.py:71-86 -----------------------
 * feat0 [2B,64,48,48], feat1 [2B,64,24,24], feat2 [2B,128,12,12] (ResNet2.forward2 of the stacked
 * left|right crops), title [B,8] (= compress_1(desc_l)), rubbish [B,264] (= compress_2(desc_l))
 * -> desc [2,B,264,145]: 8 title channels, AvgPool2d(2,1,1)+grid samples at strides 4/2/1
 * (64+64+128 channels), dustbin feature column last.  desc[0] / desc[1] are mdesc inputs of the GNN. */
int pats_fine_descriptors_f32(const float* feat0, const float* feat1, const float* feat2,
                              const float* title, const float* rubbish, int64_t B, float* desc,
                              pats_stream_t stream);

/* a15 over a capacity of B_cap rows, *B_dev of them in use (device-side count; the desc blocks of the others are left
 * untouched); channels_last != 0: the maps are torch.channels_last as for pats_fine_descriptors_nhwc_f32.  ABI 5. */
int pats_fine_descriptors_counted_f32(const float* feat0, const float* feat1, const float* feat2,
                                      const float* title, const float* rubbish, int64_t B_cap,
                                      const int64_t* B_dev, int channels_last, float* desc, pats_stream_t stream);

/* ---- a16: third-level 8x8 window gather  models/third_layer.py:121-146 -----------------------
 * feat_f0, feat_f1 [B,128,52,52]; mkpts0_c, mkpts1_c [P,2] float (x, y) coarse points in crop
 * pixels; b_ids [P] int64; kenc [128,64] (= self.kenc(kpts)[0]); rubbish [B,128,144]
 * -> out0, out1 [P,128,65] (window cell t = wy*8 + wx, dustbin feature at column 64), and the
 * rounded points the caller keeps using (p_s_out, p_t_out [P,2] int64; may be NULL).
 * Out-of-map indices (torch.gather would raise) are clamped. */
int pats_third_descriptors_f32(const float* feat_f0, const float* feat_f1, const float* mkpts0_c,
                               const float* mkpts1_c, const int64_t* b_ids, const float* kenc,
                               const float* rubbish, int64_t P, int64_t B, float* out0, float* out1,
                               int64_t* p_s_out, int64_t* p_t_out, pats_stream_t stream);

/* ---- the whole third-level step in ONE launch: a3 + a5 + a7(exp) + a17 + a18 ------------------
 * feat0, feat1 [P,D,65] (D a multiple of 32, at most 512; 128 in the reference) -> cost build (third_layer.py:156-157),
 * log_optimal_transport2(0.1*scores, 1, scale, iters) (:158), exp (:159), Compute_result (:160,
 * :184-217) and the label (:161-170).  One wave per problem; the 65x65 plan never leaves the CU
 * unless Z_out != NULL ([P,65,65] log-plan).  scale [P,64] = target areas (the OT's `ns`);
 * scale_x, scale_y [P,64] = sqrt(scale + 1e-8) as the caller computes them (:153-154).
 * whole_loss is not produced (unused at inference; use pats_compute_result_f32 for it). */
int pats_third_level_f32(const float* feat0, const float* feat1, int64_t P, int D, const float* scale,
                         const float* scale_x, const float* scale_y, const int64_t* p_s,
                         const int64_t* p_t, int iters, int outdoor, float* mkpts0_f, float* mkpts1_f,
                         float* label, uint8_t* if_matching1, float* Z_out, pats_stream_t stream);

/* a16 / the third-level step when the number of problems lives on the DEVICE (throughput mode: the merge decides P and
 * nothing reads it back): the launch covers the capacity P_cap, workgroups past *P_dev leave at once and their output rows
 * are not written.  pats_third_level_counted_f32 takes scale_x = scale_y = NULL to form sqrt(scale + 1e-8)
 * (third_layer.py:153-154) in the kernel instead of reading the caller's copies. */
int pats_third_descriptors_counted_f32(const float* feat_f0, const float* feat_f1, const float* mkpts0_c,
                                       const float* mkpts1_c, const int64_t* b_ids, const float* kenc,
                                       const float* rubbish, int64_t P_cap, const int64_t* P_dev, int64_t B,
                                       float* out0, float* out1, int64_t* p_s_out, int64_t* p_t_out,
                                       pats_stream_t stream);
int pats_third_level_counted_f32(const float* feat0, const float* feat1, int64_t P_cap, const int64_t* P_dev, int D,
                                 const float* scale, const float* scale_x, const float* scale_y, const int64_t* p_s,
                                 const int64_t* p_t, int iters, int outdoor, float* mkpts0_f, float* mkpts1_f,
                                 float* label, uint8_t* if_matching1, pats_stream_t stream);

/* a15 / a16 on CHANNELS-LAST maps (torch.channels_last: logical [B,C,H,W], memory [B,H,W,C]) - the layout a backbone run
 * under MIOpen emits natively, and the one in which the per-pixel reads of second_layer.py:73-79 and of
 * `feat.permute(0, 2, 3, 1).reshape(-1, C)` + torch.gather (third_layer.py:139-140) are contiguous runs of 256 / 512
 * bytes.  Arguments, outputs and every output bit as in pats_fine_descriptors_f32 / pats_third_descriptors_*_f32; only
 * the memory order of feat0/1/2 ([2B,48,48,64], [2B,24,24,64], [2B,12,12,128]) and feat_f0/f1 ([B,52,52,128]) differs
 * (title, rubbish, kenc as before).  Maps and desc 16-byte aligned.  P_dev may be NULL (then P_cap points exist). */
int pats_fine_descriptors_nhwc_f32(const float* feat0, const float* feat1, const float* feat2,
                                   const float* title, const float* rubbish, int64_t B, float* desc,
                                   pats_stream_t stream);
int pats_third_descriptors_nhwc_f32(const float* feat_f0, const float* feat_f1, const float* mkpts0_c,
                                    const float* mkpts1_c, const int64_t* b_ids, const float* kenc,
                                    const float* rubbish, int64_t P_cap, const int64_t* P_dev, int64_t B,
                                    float* out0, float* out1, int64_t* p_s_out, int64_t* p_t_out,
                                    pats_stream_t stream);

/* a15 / a16 on maps of a given element type (ABI 8).  A backbone run in bf16 / fp16 hands over half-precision maps; the
 * kernels widen every element to fp32 EXACTLY at the load and compute everything after it as the fp32 kernels do, in the
 * same order: desc / out0 / out1 / p_s_out / p_t_out are bit-identical to the fp32 entry points' outputs on the widened maps,
 * and stay float32.  feat* point to `dtype` elements in NCHW (channels_last == 0) or channels-last memory order, shapes as
 * above; title, rubbish, kenc, the points and the outputs are float32 / int64 as for the _f32 entry points.  B_dev / P_dev
 * may be NULL (then B_cap / P_cap rows exist); with a count, rows past it are left untouched.  PATS_MAP_F32 dispatches to
 * the fp32 kernels.  Refused before any launch (PATS_ERR_INVALID): an unknown dtype, a NULL pointer, and maps not aligned
 * to the kernels' loads - 4 bytes for NCHW maps, 16 bytes for channels-last half maps and for the fine gather's
 * channels-last maps and desc (channels-last fp32 third-level maps: 4 bytes). */
typedef enum { PATS_MAP_F32 = 0, PATS_MAP_F16 = 1, PATS_MAP_BF16 = 2 } pats_map_dtype_t;
int pats_fine_descriptors_typed(const void* feat0, const void* feat1, const void* feat2, pats_map_dtype_t dtype,
                                int channels_last, const float* title, const float* rubbish, int64_t B_cap,
                                const int64_t* B_dev, float* desc, pats_stream_t stream);
int pats_third_descriptors_typed(const void* feat_f0, const void* feat_f1, pats_map_dtype_t dtype, int channels_last,
                                 const float* mkpts0_c, const float* mkpts1_c, const int64_t* b_ids, const float* kenc,
                                 const float* rubbish, int64_t P_cap, const int64_t* P_dev, int64_t B, float* out0,
                                 float* out1, int64_t* p_s_out, int64_t* p_t_out, pats_stream_t stream);

/* The two typed gathers with the OUTPUT element type selectable as well (ABI 8, new symbols): desc / out0 / out1 point to
 * `out_dtype` elements - float32, or float16 / bfloat16 for the typed cost builds below - independent of the maps' dtype and
 * memory order.  Semantics: every output element is the float32 value pats_*_descriptors_typed writes there, rounded ONCE to
 * out_dtype, round-to-nearest-even, as tensor.to(dtype) rounds: for float16 magnitudes above 65520 become +-inf, subnormal
 * results are produced (not flushed), +-0 and +-inf pass through; for bfloat16 RNE on the upper 16 bits; a NaN stays a NaN
 * (payload unspecified).  Everything before the store is the fp32 code in its order - the widening at the load, the
 * (((a + b) + c) + d) / 4 pool, the + kenc add, the dustbin column - so the half outputs are bit-identical to the float32
 * outputs converted afterwards, and pats_cost_ot_typed / pats_third_level_typed on them to those calls on the converted
 * descriptors.  p_s_out / p_t_out do not change; with a count, rows past it are left untouched in every output type.
 * out_dtype == PATS_MAP_F32 dispatches to what the _typed entry points launch.  Half outputs of NCHW fp32 third-level maps
 * are always written by the per-point kernel (pats_set_third_gather does not apply to them).  Refused before any launch
 * (PATS_ERR_INVALID): an unknown out_dtype, what the _typed entry points refuse, and half outputs not aligned to what the
 * kernel stores - 2 bytes for NCHW maps, 16 bytes for channels-last maps.  B_cap == 0 / P_cap == 0: PATS_OK, no pointer is
 * looked at. */
int pats_fine_descriptors_typed_out(const void* feat0, const void* feat1, const void* feat2, pats_map_dtype_t dtype,
                                    int channels_last, const float* title, const float* rubbish, int64_t B_cap,
                                    const int64_t* B_dev, void* desc, pats_map_dtype_t out_dtype, pats_stream_t stream);
int pats_third_descriptors_typed_out(const void* feat_f0, const void* feat_f1, pats_map_dtype_t dtype, int channels_last,
                                     const float* mkpts0_c, const float* mkpts1_c, const int64_t* b_ids, const float* kenc,
                                     const float* rubbish, int64_t P_cap, const int64_t* P_dev, int64_t B, void* out0,
                                     void* out1, pats_map_dtype_t out_dtype, int64_t* p_s_out, int64_t* p_t_out,
                                     pats_stream_t stream);

/* The cost builds and the descriptor -> plan entry points on DESCRIPTORS of a given element type (pats_map_dtype_t; ABI 8,
 * new symbols).  Networks run under autocast hand over mdesc0 / mdesc1 and feat_f*_unfold in float16 / bfloat16; the cost
 * builds widen every element to fp32 EXACTLY at the load (subnormals, signed zeros, infinities, NaNs included) and everything
 * behind the load is the fp32 code in its order (prescale and fp16 hi + lo split, the MFMA passes, the in-kernel fp32 redo,
 * `/ sqrt(D)` then `* 0.1`, the solvers and their re-solves, the epilogues).  Every output is float32 / uint8 as for the _f32
 * entry points and bit-identical to theirs on the widened descriptors.  (Not reproduced: the reference under autocast runs
 * the einsum itself in half precision.)  scalar, ns, scale* and all outputs stay float32.  PATS_MAP_F32 runs the kernels
 * the _f32 entry points launch.  Refused before any launch (PATS_ERR_INVALID): an unknown dtype, a NULL pointer, a descriptor
 * pointer that is not aligned to its element size (all the kernels' loads need).  batch == 0 / P_cap == 0: PATS_OK, no
 * pointer is looked at.
 *   pats_cost_typed         pats_cost_f32.
 *   pats_cost_ot_typed      pats_cost_ot_f32 (col_nomatch == NULL), pats_cost_ot_flags_f32 (col_nomatch, variant 2) and
 *                           pats_cost_ot_flags_counted_f32 (batch_dev != NULL: fine level only, needs col_nomatch); workspace
 *                           as pats_cost_ot_workspace_bytes says.  Half descriptors at the fine level always take the
 *                           two-kernel path (the fused fine-level kernel reads float32 only; same bits).
 *   pats_third_level_typed  P_dev == NULL: pats_third_level_f32 (scale_x, scale_y required; Z may be NULL);
 *                           P_dev != NULL: pats_third_level_counted_f32 (scale_x = scale_y = NULL allowed; Z must be NULL). */
int pats_cost_typed(const void* d0, const void* d1, pats_map_dtype_t dtype, int64_t batch, int D, int n, int m, float* out,
                    pats_stream_t stream);
int pats_cost_ot_typed(const void* d0, const void* d1, pats_map_dtype_t dtype, int64_t batch_cap, const int64_t* batch_dev,
                       int D, int n, int m, int variant, const float* scalar, const float* ns, int iters, float bias_k,
                       float* Z, uint8_t* col_nomatch, void* workspace, size_t workspace_bytes, pats_stream_t stream);
int pats_third_level_typed(const void* feat0, const void* feat1, pats_map_dtype_t dtype, int64_t P_cap, const int64_t* P_dev,
                           int D, const float* scale, const float* scale_x, const float* scale_y, const int64_t* p_s,
                           const int64_t* p_t, int iters, int outdoor, float* mkpts0_f, float* mkpts1_f, float* label,
                           uint8_t* if_matching1, float* Z, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The steps either side of the OT path.  bool tensors are 1 byte, 0 / 1.
 * ---------------------------------------------------------------------------------------- */

/* ---- f3, throughput mode: the chunk loop of PATS.forward for a BATCH of pairs without a host read ----------------
 * Reference: models/first_layer.py:130-146 (cumsum of the matched flags, split_patches, one boolean mask + crop gather
 * + SecondLayer call per chunk), models/pats.py:33-39 (the loop; `if_nomatching1[-third_layer_set[num][1]:, :] = True`).
 * From if_nomatching1 [pairs, N] (N = height * width) this builds, on the device:
 *   sum_cycle [pairs,N] int32, cycle_num [pairs], second / third [pairs, height+1, 2]   (= pats_split_patches_device)
 *   masks [Cmax, pairs, N]      the chunk masks of first_layer.py:137-138 (1 = cell not in the chunk), chunk-major
 *   the fine level's ROW TABLE, rows ordered (chunk, pair, cell): chunk c of every pair is the contiguous block
 *     [chunk_base[c], chunk_base[c+1]) - chunk_base [Cmax+1], chunk_base[Cmax] = total rows;
 *     row_cell [rows_cap] = pair * N + cell (-1 past the total); row_crop [rows_cap] = the row's crop in the (image,
 *     patch)-ordered crop table of pats_compute_imgs_bounds_batch_f32 (crop_base [pairs+1] = first crop of every pair);
 *     row_forced [rows_cap] = 1 for the trailing rows pats.py:38-39 masks (and for padding); row_slot [Cmax, pairs*N] =
 *     the row of (chunk, cell) or -1.
 * Capacities are host-side: Cmax >= the largest chunk count (<= floor((N-1)/max_once_used) + 1 and <= height + 1),
 * rows_cap >= total rows (<= pairs * (N + (Cmax-1) * width)).  status (device int32): bit 0 = a pair had more than Cmax
 * chunks, bit 1 = more rows than rows_cap (rows were dropped) - read it when convenient, e.g. with the results. */
size_t pats_chunk_rows_workspace_bytes(int64_t pairs, int Cmax);
int pats_chunk_rows_device(const uint8_t* if_nomatching1, int64_t pairs, int height, int width, int max_once_used,
                           int Cmax, int64_t rows_cap, int32_t* sum_cycle, int32_t* cycle_num, int64_t* second,
                           int64_t* third, uint8_t* masks, int64_t* chunk_base, int64_t* crop_base, int32_t* row_cell,
                           uint8_t* row_forced, int32_t* row_crop, int32_t* row_slot, int32_t* status, void* workspace,
                           size_t workspace_bytes, pats_stream_t stream);

/* Scheduling aid, no reference counterpart: a HIP stream restricted to the compute units set in cu_mask (bit i of word
 * i / 32 = CU i; `words` 32-bit words - 8 for the 256 CUs of an MI355X).  The throughput path runs its HBM-bound stages
 * (crops, descriptor gathers) and its VALU-bound stages (the three solvers) of consecutive batches on two such streams with
 * disjoint masks (bench.py --overlap); wrap the handle with torch.cuda.ExternalStream to use it from PyTorch. */
int pats_stream_create_cu_mask(const uint32_t* cu_mask, int words, pats_stream_t* stream);
int pats_stream_destroy(pats_stream_t stream);

/* Profiling aid, no reference counterpart: launches an empty kernel named pats::profile_marker_kernel on `stream`, so that
 * a kernel trace can be cut to the region between two markers (bench.py brackets its timed steps with it). */
int pats_profile_marker(int tag, pats_stream_t stream);

/* SecondLayer.merge_patches_new / _old (models/second_layer.py:137-238) for every chunk of every pair of the row table
 * above, in the reference's order: chunk blocks one after the other (the chunks of a pair couple through scores_back,
 * pats.py:32,37), each block over all pairs at once.  trust_score / if_nomatching1_L2 [rows_cap,144] are updated in place
 * like the reference; scores_back [pairs, N, 16, 9] fp64 (zeros before the first chunk, pats.py:32: zero_scores_back != 0
 * clears it here); out [rows_cap,144] =
 * the returned if_nomatching with pats.py:38-39 applied (row_forced) and padding rows all "no match". */
size_t pats_merge_batch_workspace_bytes(int64_t pairs, int H, int W);
int pats_merge_patches_batch(int merge_new, int Cmax, int64_t pairs, int H, int W, int64_t rows_cap,
                             const int64_t* chunk_base, const int32_t* row_cell, const int32_t* row_slot,
                             const uint8_t* row_forced, float* trust_score, uint8_t* if_nomatching1_L2,
                             double* scores_back, int zero_scores_back, uint8_t* out, void* workspace,
                             size_t workspace_bytes, pats_stream_t stream);

/* The same merges for chunks [c_lo, c_hi) of the row table only, on tensors that hold table rows row_origin .. row_origin +
 * rows_local (trust_score, if_nomatching1_L2, out [rows_local,144]): PATS.forward's chunk loop (models/pats.py:33-39) walked
 * chunk by chunk - one launch per chunk, scores_back handed from call to call (zero_scores_back != 0 on the first,
 * pats.py:32), pats.py:38-39 applied through row_forced.  Rows of `out` outside the walked blocks read "no match". */
int pats_merge_patches_chunks(int merge_new, int Cmax, int c_lo, int c_hi, int64_t pairs, int H, int W, int64_t row_origin,
                              int64_t rows_local, const int64_t* chunk_base, const int32_t* row_cell, const int32_t* row_slot,
                              const uint8_t* row_forced, float* trust_score, uint8_t* if_nomatching1_L2, double* scores_back,
                              int zero_scores_back, uint8_t* out, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* PATS.forward's chunk loop (models/pats.py:33-78) walked chunk by chunk: everything between the network callbacks of ONE chunk in
 * two calls (csrc/chunk_walk.cpp - each runs the entry points above in the reference's order on `stream`; what they save is host
 * time).  B = the chunk's rows; the row table is pats_chunk_rows_device's, c the chunk, row_origin = chunk_base[c] (host copy).
 *   fine tail: second_layer.py:100-122 + pats.py:37-39,53-58.  In: the chunk's descriptors d0, d1 [B,264,145], one (device 1.0f),
 *   ns = scale_x * scale_y [B,144], the two scale heads.  Out: Z [B,145,145] (+ ln bias_k), col_nomatch / row_nomatch [B,144], the
 *   expansion's six outputs, merged [B,144] (the returned if_nomatching, tail rows forced), mkpts0 / mkpts1 [144 B,2], b_ids [144 B],
 *   *P_dev.  trust and row_nomatch are updated in place by the merge as in the reference.  wait_before_merge / record_after_merge:
 *   optional hipEvent_t handles - the stream waits for the first right before the merge and records the second right behind it (the
 *   merges of a pair are ordered, pats.py:37; with consecutive chunks on different streams only they need to wait for each other).
 *   third tail: third_layer.py:153-170 + pats.py:59-78.  In: the third level's descriptors over the capacity P_cap = 144 B with the
 *   count *P_dev, scale [P_cap,64], the rounded points, merged / points2 of the fine tail, the chunk's mask [h w] (level-0 flags),
 *   Compute_imgs' pts_new / scales [1,h w,2], `ones` = B bytes of 1.  Out: the third level's four outputs, if_nomatching16 [B,2304],
 *   pts16 [B,2304,2], matches_l / matches_r [2304 B,2], match_row, *M_dev. */
size_t pats_chunk_fine_tail_workspace_bytes(int64_t B, int64_t pairs, int H, int W);
int pats_chunk_fine_tail_f32(const float* d0, const float* d1, int64_t B, const float* one, const float* ns, int iters, float bias_k,
                             const float* scale_x, const float* scale_y, int merge_new, int Cmax, int c, int64_t pairs, int H, int W,
                             int64_t row_origin, const int64_t* chunk_base, const int32_t* row_cell, const int32_t* row_slot,
                             const uint8_t* row_forced, double* scores_back, int first_chunk, float* Z, uint8_t* col_nomatch,
                             float* trust, float* core, float* points, float* x_scale, float* y_scale, int64_t* bound,
                             uint8_t* row_nomatch, uint8_t* merged, float* mkpts0, float* mkpts1, int64_t* b_ids, int64_t* P_dev,
                             void* wait_before_merge, void* record_after_merge, void* workspace, size_t workspace_bytes,
                             pats_stream_t stream);
size_t pats_chunk_third_tail_workspace_bytes(int64_t B, int h, int w);
int pats_chunk_third_tail_f32(const float* feat0, const float* feat1, int64_t P_cap, const int64_t* P_dev, const float* scale,
                              const int64_t* p_s, const int64_t* p_t, int iters, int outdoor, const uint8_t* merged,
                              const float* points2, int64_t B, const uint8_t* chunk_mask, int h, int w, const float* pts_new,
                              const float* scales, const uint8_t* ones, float* mkpts0_f, float* mkpts1_f, float* label,
                              uint8_t* if_matching1, uint8_t* if_nomatching16, float* pts16, float* matches_l, float* matches_r,
                              int32_t* match_row, int64_t* M_dev, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* SecondLayer.merge_patches_new (merge_new != 0, reference models/second_layer.py:193-240) and
 * merge_patches_old (merge_new == 0, :137-191): resolves every 8-px cell among the up to nine 96x96
 * windows covering it.  Like the reference it works in place on trust_score [B,144] (border weighting
 * :194-198, and -10000 on matching cells for "new" :201) and on if_nomatching1_L2 [B,144] (:199-200),
 * and writes this chunk's scores into scores_back [batch_num, H/32*W/32, 16, 9] (fp64, :211; the
 * "new" variant reads the other patches' entries left there by earlier chunks, pats.py:32,37).
 * `out` [B,144] is the returned if_nomatching (rows = unmasked entries of if_nomatching1_L1, in
 * order).  The reference raises when the number of unmasked coarse patches differs from B; here
 * surplus patches are ignored and missing ones leave their rows "no match" - host wrappers validate. */
size_t pats_merge_workspace_bytes(int64_t B, int H, int W, int batch_num);
int pats_merge_patches(int merge_new, int64_t B, float* trust_score, int H, int W, int batch_num,
                       const uint8_t* if_nomatching1_L1, uint8_t* if_nomatching1_L2, double* scores_back,
                       uint8_t* out, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* Workspace of the order-preserving compactions below over n flags. */
size_t pats_compact_workspace_bytes(int64_t n);

/* Third-level inputs (reference models/pats.py:53-58): for every L2 cell with if_nomatching == 0, in
 * (row, cell) order, mkpts0 = ((cell % 12) * 4 + 2, (cell / 12) * 4 + 2) * 2, mkpts1 =
 * round(pts * 4)[(1, 0)] * 2 (round half to even) and the patch row b_ids.  Writes at most `capacity`
 * rows; *count (device int64) receives the number of surviving cells P. */
int pats_third_inputs_f32(const uint8_t* if_nomatching, const float* pts, int64_t B, float* mkpts0,
                          float* mkpts1, int64_t* b_ids, int64_t capacity, int64_t* count, void* workspace,
                          size_t workspace_bytes, pats_stream_t stream);

/* Scatter of the third-level results onto the 48x48 sub-cell grid (reference models/pats.py:59-67):
 * pts16 [B,2304,2] takes mkpts1_f [P,16,2] where the L2 cell survived (else the L2 point), and
 * if_nomatching16 [B,2304] = L2 flag OR label < -9.9; layout [B,12,4,12,4].  `label` is read with a
 * stride (2 for the reference's label[:, 0] of a [P*16,2] tensor). */
int pats_refine_scatter_f32(const uint8_t* if_nomatching, const float* pts, const float* mkpts1_f,
                            const float* label, int label_stride, int64_t B, int64_t P,
                            uint8_t* if_nomatching16, float* pts16, void* workspace,
                            size_t workspace_bytes, pats_stream_t stream);

/* get_result with layer_num = 2 (reference utils/utils.py:189-213, called at models/pats.py:73):
 * level 0 has batch_size rows of patch_size0[1]*patch_size0[2] cells of patch_size0[0] px, level 1 has
 * `rows1` rows (one per surviving level-0 cell, in order) of patch_size1[1]*patch_size1[2] sub-cells.
 * scale1_cell_stride = 2: scale1 is [rows1, n1, 2] as the reference materialises it; 0: scale1 is
 * [rows1, 2], one scale per row (what pats.py:70 repeats).  Output order = reference (row, sub-cell);
 * at most `capacity` rows are written, *count (device int64) receives M.  fp32, operation order of the
 * reference.  Workspace: pats_get_result_workspace_bytes(batch_size*n0, rows1, n1).
 * rows1 may exceed the number of surviving level-0 cells K (a capacity-sized tensor): rows K .. rows1 - 1 emit
 * nothing, and the first M_true slots (the unflagged sub-cells of rows 0 .. K - 1) are the matches.  *count is
 * the total of the level-1 flag scan over ALL rows1 rows: it equals M_true only when the rows past K are fully
 * flagged (what pats_refine_scatter_f32 / the batch merge leave there).  Otherwise *count = M_true + their
 * unflagged sub-cells, and the slots M_true .. *count - 1 stay unwritten - a caller that cannot guarantee the
 * flags must not read them.  The same holds for the pats_get_result_chunks_* entries and their match_row /
 * match_conf. */
size_t pats_get_result_workspace_bytes(int64_t cells0, int64_t rows1, int64_t cells1);
int pats_get_result_f32(int batch_size, const uint8_t* if_nomatching0, const uint8_t* if_nomatching1,
                        int64_t rows1, const float* average_point0, const float* average_point1,
                        const float* scale0, const float* scale1, int64_t scale1_cell_stride,
                        const int* patch_size0, const int* patch_size1, const uint8_t* left_choice0,
                        const uint8_t* left_choice1, float* matches_l, float* matches_r, int64_t capacity,
                        int64_t* count, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* get_result for every (chunk, pair) of a batch in ONE call (models/pats.py:68-73, utils/utils.py:189-213): level-0
 * batch = the Cmax * pairs chunk masks, level-1 rows = the row table of pats_chunk_rows_device.  pts_new, scales
 * [pairs, N, 2] are the per-pair tensors of Compute_imgs (not expanded over the chunks, not flipped - pats.py:71's
 * `.flip(dims=[2]) / 32.0` happens on load), pts16 [rows_cap, n1, 2] un-flipped (`/ 2.0` on load), the level-1 scale of a
 * row is the level-0 scale of its cell (pats.py:70).  match_row [capacity] (optional) = the row of every match: row_cell
 * [match_row] / N is its pair.  Same arithmetic and output order as pats_get_result_f32 on the expanded tensors. */
int pats_get_result_chunks_f32(int Cmax, int64_t pairs, const uint8_t* masks, const uint8_t* if_nomatching16,
                               int64_t rows_cap, const float* pts_new, const float* pts16, const float* scales,
                               const int* patch_size0, const int* patch_size1, const uint8_t* left_choice0,
                               const uint8_t* left_choice1, float* matches_l, float* matches_r, int32_t* match_row,
                               int64_t capacity, int64_t* count, void* workspace, size_t workspace_bytes,
                               pats_stream_t stream);

/* The matches of a batch grouped BY PAIR on the device (ABI 5; throughput mode's hand-over, no reference counterpart: the
 * reference runs one pair at a time).  Input = what pats_get_result_chunks_f32 wrote (matches in (chunk, pair, patch, sub-cell)
 * order, match_row, the count *M_dev) + the row table's row_cell / chunk_base; output = the same matches with every pair's list
 * contiguous and in the reference's order (its chunks one after the other), pair_off [pairs + 1] int64: pair p owns rows
 * [pair_off[p], pair_off[p + 1]) of out_l / out_r.  No host read. */
size_t pats_matches_by_pair_workspace_bytes(int Cmax, int64_t pairs);
int pats_matches_by_pair_f32(const float* matches_l, const float* matches_r, const int32_t* match_row, const int64_t* M_dev,
                             const int32_t* row_cell, const int64_t* chunk_base, int Cmax, int64_t pairs, int N,
                             float* out_l, float* out_r, int64_t* pair_off, void* workspace, size_t workspace_bytes,
                             pats_stream_t stream);
/* The same with the step's counters appended: pair_off has pairs + 4 entries - the pairs + 1 offsets, then M, P (*P_dev: the
 * third-level problem count of the step, may be null) and the row table's status - a batch's hand-over is ONE device-to-host copy. */
int pats_matches_by_pair_summary_f32(const float* matches_l, const float* matches_r, const int32_t* match_row, const int64_t* M_dev,
                                     const int32_t* row_cell, const int64_t* chunk_base, int Cmax, int64_t pairs, int N,
                                     float* out_l, float* out_r, int64_t* pair_off, const int64_t* P_dev, const int32_t* status,
                                     void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ---- ragged batches (ABI 7): pairs of DIFFERENT grids in one throughput batch --------------------------------------------
 * Pair p has the coarse grid h_p x w_p (N_p = h_p w_p cells) and the images [32 h_p, 32 w_p, 3].  Every per-cell tensor of the
 * batch is PACKED over cells: pair p owns cells [cell_base[p], cell_base[p+1]) (if_nomatching1, sum_cycle, pts_new, scales,
 * scores_back [sum N, 16, 9], the chunk masks and row_slot [Cmax, sum N]); a uniform batch is the special case cell_base[p] =
 * p N, i.e. exactly the layout of the entry points above.  The table is handed over twice: in host memory (validated before
 * any launch, sizes the launches) and in device memory (what the kernels read).  Bad tables - null arrays, pairs < 1, h_p or
 * w_p <= 0 or N_p >= 10000 (the crop sequence img * 10000 + patch), cell_base[0] != 0 or cell_base[p+1] - cell_base[p] !=
 * N_p - are refused with PATS_ERR_INVALID. */
typedef struct pats_pair_table {
    int64_t pairs;
    const int32_t* shape_host;       /* [pairs, 2] (h_p, w_p), host memory */
    const int64_t* cell_base_host;   /* [pairs + 1], host memory */
    const int32_t* shape;            /* the same two arrays in device memory */
    const int64_t* cell_base;
    const int64_t* img_base;         /* [pairs] device: offset in elements of pair p's image in the flat left / right stores */
} pats_pair_table_t;

/* pats_chunk_rows_device for a ragged batch: each pair is planned on its own grid with the chunk cap of first_layer.py:131-135
 * (2 w_p when if_local, 512 otherwise).  second / third [pairs, max h + 1, 2]; masks / row_slot [Cmax, sum N]; row_cell = the
 * packed cell; row_pair [rows_cap] = the row's pair (-1 past the total).  1 <= Cmax <= max h + 1.  Workspace:
 * pats_chunk_rows_workspace_bytes(pairs, Cmax). */
int pats_chunk_rows_ragged(const pats_pair_table_t* tab, const uint8_t* if_nomatching1, int if_local, int Cmax, int64_t rows_cap,
                           int32_t* sum_cycle, int32_t* cycle_num, int64_t* second, int64_t* third, uint8_t* masks,
                           int64_t* chunk_base, int64_t* crop_base, int32_t* row_cell, int32_t* row_pair, uint8_t* row_forced,
                           int32_t* row_crop, int32_t* row_slot, int32_t* status, void* workspace, size_t workspace_bytes,
                           pats_stream_t stream);
/* pats_compute_imgs_bounds_batch_f32 / pats_left_crops_counted_f32 / pats_tensor_resize_hwc_counted_f32 for a ragged batch:
 * per-cell inputs and outputs packed, bound5 [sum N, 5]; pair p's images are read at img_base[p] with its own 32 h_p x 32 w_p,
 * and every read outside them is the reference's zero padding (utils.py:1352), whatever memory lies beside them. */
int pats_compute_imgs_bounds_ragged_f32(const pats_pair_table_t* tab, const float* x_scale, const float* y_scale,
                                        const float* average_point, const uint8_t* if_nomatching, int64_t* bound5, int64_t* K_img,
                                        int64_t* K_total, float* x_scale_new, float* y_scale_new, float* average_new,
                                        pats_stream_t stream);
int pats_left_crops_ragged_f32(const pats_pair_table_t* tab, const float* left, const int64_t* bound5, int64_t K_cap,
                               const int64_t* K_dev, float* out, pats_stream_t stream);
int pats_tensor_resize_hwc_ragged_f32(const pats_pair_table_t* tab, const float* right, int margin, const int64_t* bound5,
                                      int64_t K_cap, const int64_t* K_dev, float* out, int32_t* status, pats_stream_t stream);

/* ---- a13 / a14 on images of any element type, crops in the backbone's format --------------------------------------------
 * The images (left / right HWC stores, tensor_resize's NCHW input) hold `dtype` elements.  Each element is widened to fp32
 * EXACTLY at the load, and the crop is computed as the _f32 kernels compute it, in the same order: an fp32 crop is
 * bit-identical to the _f32 entry points' crop of the images converted to float32.  The format then applies per element,
 * in fp32: with `normalize`, (x - mean[c]) / std[c] (a subtraction, then an IEEE division: torchvision's Normalize), then ONE
 * rounding to `dtype` (round-to-nearest-even).  layout hwc = [K,96,96,3], chw = [K,3,96,96] ([K,C,96,96] for tensor_resize,
 * whose output is always chw).  PATS_IMG_U8 output: left crops of uint8 images only, not normalised (exact copies).  A crop
 * that tensor_resize refuses (status) is written as the format's value of a zero pixel.
 * tab: a ragged batch (n_img, H, W, height, width are then unused), or NULL for n_img uniform images.  K_dev: NULL = K_cap
 * crops; else the crops run over the capacity K_cap and rows >= *K_dev are left untouched.  Refused before any launch
 * (PATS_ERR_INVALID): an unknown image dtype, output dtype or layout; uint8 output for right crops / tensor_resize, of other
 * images or with normalisation; with normalisation, a non-finite mean / std or std == 0 (tensor_resize: also C != 3); NULL
 * pointers; images not aligned to their element size; out not 16-byte aligned.  PATS_CROPS_NT applies to every format. */
typedef enum { PATS_IMG_F32 = 0, PATS_IMG_F16 = 1, PATS_IMG_BF16 = 2, PATS_IMG_U8 = 3 } pats_img_dtype_t;
typedef enum { PATS_CROP_HWC = 0, PATS_CROP_CHW = 1 } pats_crop_layout_t;
typedef struct pats_crop_format {
    int32_t dtype;        /* pats_img_dtype_t of the crops */
    int32_t layout;       /* pats_crop_layout_t */
    int32_t normalize;    /* 0 / 1 */
    float mean[3];
    float std[3];
} pats_crop_format_t;
int pats_left_crops_typed(const pats_pair_table_t* tab, const void* left, pats_img_dtype_t dtype, int n_img, int H, int W,
                          int height, int width, const int64_t* bound5, int64_t K_cap, const int64_t* K_dev,
                          const pats_crop_format_t* fmt, void* out, pats_stream_t stream);
int pats_tensor_resize_hwc_typed(const pats_pair_table_t* tab, const void* right, pats_img_dtype_t dtype, int n_img, int H, int W,
                                 int margin, const int64_t* bound5, int64_t K_cap, const int64_t* K_dev,
                                 const pats_crop_format_t* fmt, void* out, int32_t* status, pats_stream_t stream);
int pats_tensor_resize_typed(const void* input, pats_img_dtype_t dtype, int n_img, int C, int Hp, int Wp, const int64_t* bound,
                             int64_t K_cap, const int64_t* K_dev, const pats_crop_format_t* fmt, void* out, int32_t* status,
                             pats_stream_t stream);
/* pats_merge_patches_batch for a ragged batch (row table of pats_chunk_rows_ragged; scores_back packed [sum N, 16, 9]). */
size_t pats_merge_ragged_workspace_bytes(int64_t total_cells);
int pats_merge_patches_ragged(const pats_pair_table_t* tab, int merge_new, int Cmax, int64_t rows_cap, const int64_t* chunk_base,
                              const int32_t* row_cell, const int32_t* row_pair, const int32_t* row_slot, const uint8_t* row_forced,
                              float* trust_score, uint8_t* if_nomatching1_L2, double* scores_back, int zero_scores_back,
                              uint8_t* out, void* workspace, size_t workspace_bytes, pats_stream_t stream);
/* pats_get_result_chunks_f32 for a ragged batch: level-0 patch_size of pair p is (32, h_p, w_p); masks [Cmax, sum N],
 * pts_new / scales packed [sum N, 2].  Workspace: pats_get_result_workspace_bytes(Cmax * sum N, rows_cap, n1). */
int pats_get_result_chunks_ragged_f32(const pats_pair_table_t* tab, int Cmax, const uint8_t* masks, const uint8_t* if_nomatching16,
                                      int64_t rows_cap, const float* pts_new, const float* pts16, const float* scales,
                                      const int* patch_size1, const uint8_t* left_choice0, const uint8_t* left_choice1,
                                      float* matches_l, float* matches_r, int32_t* match_row, int64_t capacity, int64_t* count,
                                      void* workspace, size_t workspace_bytes, pats_stream_t stream);
/* pats_matches_by_pair_summary_f32 with the pair of a match taken from the row table's row_pair (any batch, ragged or not).
 * status may be null: pair_off then holds the pairs + 1 offsets only (as pats_matches_by_pair_f32), and P_dev is ignored. */
int pats_matches_by_row_pair_summary_f32(const float* matches_l, const float* matches_r, const int32_t* match_row,
                                         const int64_t* M_dev, const int32_t* row_pair, const int64_t* chunk_base, int Cmax,
                                         int64_t pairs, float* out_l, float* out_r, int64_t* pair_off, const int64_t* P_dev,
                                         const int32_t* status, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Image front end (ABI 8, symbols added): the step in FRONT of the throughput path - what the reference's data set classes do to a
 * decoded image on the CPU (datasets/yfcc.py:33-60, datasets/scannet.py:40-55): the centre crop and resize of Resize_img
 * (utils/utils.py:1118-1131), the zero pad of cv2.copyMakeBorder up to a canvas that is a multiple of 32 and common to the pair, and
 * the matching change to the intrinsics.  One launch turns every raw uint8 [h0, w0, 3] image of a batch - each its own allocation,
 * of any size - into its canvas inside the flat left / right stores of a ragged batch (pats_pair_table_t.img_base), pad included.
 * What it is not: a decoder, a normalisation or a grayscale conversion (those belong to the backbone and pats_crop_format_t).
 *
 * WHAT HAS BEEN CHECKED.  The resampling below is written from a reading of OpenCV's portable (non-SIMD-specific) uint8 path of
 * cv2.resize with INTER_LINEAR.  It has NOT been run against any OpenCV build, and some builds route cv2.resize through IPP or a
 * HAL with other rounding: no bit parity with an installed OpenCV is claimed.  Checked on the CPU: a numpy restatement of the
 * rules below stays within 0.80 grey levels of float64 bilinear interpolation (half-pixel centres, align_corners = False) on
 * eight shapes from 2 x 2 to 480 x 640, up- and downscaling, and maps constant 0 and constant 255 images to themselves; the
 * kernel's output is bit-equal to that restatement (tests/test_prepare_gpu.py).
 *
 * Per image, ON THE HOST, in Python floats (IEEE double) exactly as the reference's lines - int() truncates toward zero:
 *   target     from `size`: s = size / max(h0, w0), w_t = int(w0 * s), h_t = int(h0 * s) (yfcc.py:35-37); or given as (w_t, h_t).
 *              Both at least 1
 *   window     if w0 / w_t < h0 / h_t:  gap = int((h0 - w0 / w_t * h_t) / 2), rows [gap, h0 - gap), all columns
 *              otherwise:               gap = int((w0 - h0 / h_t * w_t) / 2), columns [gap, w0 - gap), all rows
 *              its size is (h_c, w_c) (Resize_img's slices)
 *   canvas     per image ceil32(h_t) x ceil32(w_t); per pair the maximum of its two images' in each axis (yfcc.py:43-60); or one
 *              fixed (H, W) for all pairs (scannet.py:52-53), which every target must fit.  The image sits at the top left; the
 *              rest of the canvas is zero
 * ON THE DEVICE the window S [h_c, w_c, 3] is resampled to [h_t, w_t, 3]:
 *   per axis   with sn source and dn destination samples:  inv = double(dn) / double(sn), scale = 1.0 / inv (the table's scale_x /
 *              scale_y).  For destination sample d:
 *                f = float32((d + 0.5) * scale - 0.5)      evaluated in float64 without contraction, then rounded once
 *                s = floor(f), f = f - s (float32);  if s < 0: s = 0, f = 0;  if s >= sn - 1: s = sn - 1, f = 0
 *                second tap t = min(s + 1, sn - 1)
 *                a0 = rint((1.0f - f) * 2048.0f), a1 = rint(f * 2048.0f)      float32 operations, ties to even
 *   passes     a = the x coefficients of column d, b = the y coefficients of row y (taps y0, y1), int32 arithmetic:
 *                Hsum[r][d][c] = S[r][s][c] * a0 + S[r][t][c] * a1
 *                out[y][d][c] = (((b0 * (Hsum[y0][d][c] >> 4)) >> 16) + ((b1 * (Hsum[y1][d][c] >> 4)) >> 16) + 2) >> 2, clamped
 *                to [0, 255]
 *   halving    if w_c == 2 w_t AND h_c == 2 h_t the 2 x 2 mean replaces bilinear:
 *                out[y][x][c] = (S[2y][2x][c] + S[2y][2x+1][c] + S[2y+1][2x][c] + S[2y+1][2x+1][c] + 2) >> 2
 *              A halving in one axis only stays bilinear
 *   bgr        with bgr = 1 output channel c reads source channel 2 - c (the reference's [:, :, [2, 1, 0]])
 *   dtype      the stores' element type: PATS_IMG_U8, _F32, _F16 or _BF16 - 0 .. 255 is exact in all four
 * Intrinsics (host, numpy float64, the reference's operation order; pats_amd/ops.py prepare_intrinsics), K the 3 x 3 of the raw image:
 *   "ratio"    yfcc.py:39-42 with Get_resize_ratio (utils.py:943-957) on (w0, h0) and (w_t, h_t) as floats:  h_w = h_t / w_t;
 *              if w0 / w_t < h0 / h_t:  r = w_t / w0, add = (0, (h0 - w0 * h_w) / 2);  otherwise r = h_t / h0,
 *              add = ((w0 - h0 / h_w) / 2, 0).  K' = r * K, K'[2][2] = 1, K'[0:2][2] -= add * r.  `add` is the reference's FLOAT gap,
 *              not the integer gap of the crop
 *   "axes"     scannet.py:54-55 with scale_intrinsics (utils/metrics.py:6-8):  K' = diag(1 / sx, 1 / sy, 1) K (a matrix product),
 *              sx = float(w0) / w_t, sy = float(h0) / h_t
 *   norm       [pairs,8] float32 = (cy_l, cx_l, 1 / fy_l, 1 / fx_l, cy_r, cx_r, 1 / fy_r, 1 / fx_r) of K'_l, K'_r - each formed in
 *              float64 and rounded once to float32: the `norm` of the per-pair stages below
 *   thr        [pairs] float32 = threshold / mean(K'_l[0][0], K'_r[1][1], K'_l[0][0], K'_r[1][1]) (metrics.py:36-37; numpy's mean of
 *              the four, float64, rounded once)
 *
 * pats_prepare_images_u8 - one launch for all n_img images.  The table is handed over twice, as pats_pair_table_t is: images_host
 * (host memory; validated before the launch, sizes it) and images (the same bytes in device memory; what the kernel reads).
 * left / right: the stores, left_elems / right_elems elements of `dtype` long; image i's canvas [H, W, 3] is written - every
 * element of it, pad included, nothing else - at element dst of the store `side` names.  No workspace, no host read, no allocation:
 * the call can be captured in a graph.
 * Refused before the launch (PATS_ERR_INVALID; pats_last_error names the image): a null images_host / images / left / right or a
 * null src; images off 8 bytes, left / right off 16; an unknown dtype; n_img outside 1 .. 65535; a source or canvas side above
 * pats_prepare_images_max_side() (16384); a window that is empty or leaves its source; a canvas side that is not a positive
 * multiple of 32; a target below 1 or larger than its canvas; side or bgr not 0 / 1; scale_x / scale_y not the definition's
 * double; a canvas that leaves its store or does not start on a 16-byte boundary. */
typedef struct pats_prepare_image {
    const uint8_t* src;      /* device: the raw image [h0, w0, 3] uint8, contiguous */
    int64_t dst;             /* offset in ELEMENTS of the canvas in its store: pats_pair_table_t.img_base of the image's slot */
    double scale_x;          /* 1.0 / (double(w_t) / double(w_c)) */
    double scale_y;          /* 1.0 / (double(h_t) / double(h_c)) */
    int32_t h0, w0;          /* the raw image */
    int32_t y0, x0;          /* the window's first row and column */
    int32_t h_c, w_c;        /* the window's size */
    int32_t h_t, w_t;        /* the target */
    int32_t H, W;            /* the canvas */
    int32_t side;            /* 0: the left store, 1: the right store */
    int32_t bgr;             /* 0 / 1 */
} pats_prepare_image_t;
int64_t pats_prepare_images_max_side(void);
int pats_prepare_images_u8(const pats_prepare_image_t* images_host, const pats_prepare_image_t* images, int64_t n_img, void* left,
                           int64_t left_elems, void* right, int64_t right_elems, pats_img_dtype_t dtype, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-match confidence (ABI 8, symbols added).  For third-level problem p and centre source cell k in 0..15 (row r of the 8x8
 * grid inside [2:6, 2:6], in Compute_result's order), with S = exp(Z) the [65,65] plan:
 *     rowmass = sum of S[r, :] over all 65 columns, dustbin included           (first term of third_layer.py:213)
 *     winmass = sum of S[r, c] over the 5x5 window around argmax_c S[r, :64], zero outside the 8x8 grid   (:212)
 *     conf[p,k] = winmass / rowmass        float32, at most 1; computed for all 16 cells whatever label / if_matching1 say
 * The reference folds rowmass - winmass into a training loss; nothing else of it is kept.  Every entry below is the entry it is
 * named after with the extra pointer(s): it refuses a null or not 4-byte aligned confidence pointer before any launch
 * (pats_last_error names the argument), then runs the same implementation with the confidence instantiation of the same kernel
 * - every other output has the bits of the plain call.  Workspaces are those of the plain entries.
 *   pats_third_level_typed_conf          conf [P_cap,16] beside mkpts1_f (rows past *P_dev not written); a problem the guard
 *                                        sends to a re-solve gets the confidence of the re-solved plan
 *   pats_compute_result_ws_conf_f32      conf [P,16] from a plan in memory
 *   pats_refine_scatter_conf_f32         conf [P,16] -> conf16 [B,2304] by pts16's permutation; 0 where if_nomatching16 is set.
 *                                        conf may be null when P == 0
 *   pats_get_result_chunks(_ragged)_conf_f32   conf16 [rows_cap,n1] -> match_conf [capacity], the slots of matches_l / matches_r
 *   pats_matches_by_(row_)pair_summary_conf_f32   match_conf [M] -> out_conf, regrouped with the matches.  status may be null in
 *                                        both: pair_off then holds the pairs + 1 offsets only and P_dev is ignored */
int pats_third_level_typed_conf(const void* feat0, const void* feat1, pats_map_dtype_t dtype, int64_t P_cap, const int64_t* P_dev,
                                int D, const float* scale, const float* scale_x, const float* scale_y, const int64_t* p_s,
                                const int64_t* p_t, int iters, int outdoor, float* mkpts0_f, float* mkpts1_f, float* label,
                                uint8_t* if_matching1, float* Z, float* conf, pats_stream_t stream);
int pats_compute_result_ws_conf_f32(const float* scores, int input_is_log, int64_t P, const float* scale_x,
                                    const float* scale_y, const int64_t* p_s, const int64_t* p_t, int outdoor,
                                    float* mkpts0_f, float* mkpts1_f, float* whole_loss, float* label,
                                    uint8_t* if_matching1, float* conf, void* workspace, size_t workspace_bytes,
                                    pats_stream_t stream);
int pats_refine_scatter_conf_f32(const uint8_t* if_nomatching, const float* pts, const float* mkpts1_f, const float* label,
                                 int label_stride, const float* conf, int64_t B, int64_t P, uint8_t* if_nomatching16,
                                 float* pts16, float* conf16, void* workspace, size_t workspace_bytes, pats_stream_t stream);
int pats_get_result_chunks_conf_f32(int Cmax, int64_t pairs, const uint8_t* masks, const uint8_t* if_nomatching16,
                                    int64_t rows_cap, const float* pts_new, const float* pts16, const float* scales,
                                    const float* conf16, const int* patch_size0, const int* patch_size1,
                                    const uint8_t* left_choice0, const uint8_t* left_choice1, float* matches_l,
                                    float* matches_r, float* match_conf, int32_t* match_row, int64_t capacity,
                                    int64_t* count, void* workspace, size_t workspace_bytes, pats_stream_t stream);
int pats_get_result_chunks_ragged_conf_f32(const pats_pair_table_t* tab, int Cmax, const uint8_t* masks,
                                           const uint8_t* if_nomatching16, int64_t rows_cap, const float* pts_new,
                                           const float* pts16, const float* scales, const float* conf16,
                                           const int* patch_size1, const uint8_t* left_choice0, const uint8_t* left_choice1,
                                           float* matches_l, float* matches_r, float* match_conf, int32_t* match_row,
                                           int64_t capacity, int64_t* count, void* workspace, size_t workspace_bytes,
                                           pats_stream_t stream);
int pats_matches_by_pair_summary_conf_f32(const float* matches_l, const float* matches_r, const float* match_conf,
                                          const int32_t* match_row, const int64_t* M_dev, const int32_t* row_cell,
                                          const int64_t* chunk_base, int Cmax, int64_t pairs, int N, float* out_l, float* out_r,
                                          float* out_conf, int64_t* pair_off, const int64_t* P_dev, const int32_t* status,
                                          void* workspace, size_t workspace_bytes, pats_stream_t stream);
int pats_matches_by_row_pair_summary_conf_f32(const float* matches_l, const float* matches_r, const float* match_conf,
                                              const int32_t* match_row, const int64_t* M_dev, const int32_t* row_pair,
                                              const int64_t* chunk_base, int Cmax, int64_t pairs, float* out_l, float* out_r,
                                              float* out_conf, int64_t* pair_off, const int64_t* P_dev, const int32_t* status,
                                              void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair top-K (ABI 8, symbols added): each pair's K most confident matches out of the regrouped hand-over
 * (pats_matches_by_(row_)pair_summary_conf_f32: matches_l / matches_r [cap,2], conf [cap], pair_off [pairs + 1] - a longer buffer
 * with the summary behind the offsets is fine), exact and deterministic, ONE launch for the whole batch, no host read.
 * For pair p: lo = pair_off[p], hi = pair_off[p + 1] (both clamped to [0, cap] on the device; hi <= lo is an empty pair - a stale
 * pair_off never causes a read outside the arrays), n = hi - lo, i in 0..n-1 the position inside the pair's list.
 *   key(i)      = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), b = the 32 bits of conf[lo + i]: the order-preserving map of float32
 *                 onto uint32.  On [0, 1] a larger key is a larger confidence; +inf and a positive NaN rank ABOVE every number
 *                 (a broken confidence shows up first instead of vanishing), negative values and negative NaNs below 0.0
 *   eligible    use_min_conf == 0, or key(i) >= key(min_conf) - for finite non-negative values conf >= min_conf, inclusive
 *   ranking     eligible matches by key descending, ties by i ascending (a stable descending sort)
 *   top_count   [pairs] int64: min(K, number of eligible matches)
 *   j <  count  top_idx[p,j] = the i of rank j; top_l[p,j], top_r[p,j], top_conf[p,j] = matches_l[lo+i], matches_r[lo+i],
 *               conf[lo+i], bit for bit
 *   j >= count  top_idx = -1, top_l = top_r = top_conf = 0.0: every call defines every byte of every output
 * top_l, top_r [pairs,K,2] float32, top_conf [pairs,K] float32, top_idx [pairs,K] int32.  1 <= K <= pats_topk_by_pair_max_k()
 * (8192: the composites of one pair are sorted in 64 KB of LDS).  cap = the rows the input arrays hold (cap == 0: every pair
 * empty, outputs defined).  Refused before any launch (pats_last_error names the argument): a null pointer; matches_l / matches_r /
 * top_l / top_r off 8 bytes (read and written as float2), conf / top_conf / top_idx off 4, pair_off / top_count off 8; pairs < 1,
 * cap < 0 (or >= 2^31 - 1: top_idx is int32), K < 1, K > max_k; use_min_conf with a NaN or negative min_conf; a workspace smaller
 * than pats_topk_by_pair_workspace_bytes (0 today: the kernel keeps everything in LDS; workspace may then be null). */
int64_t pats_topk_by_pair_max_k(void);
size_t pats_topk_by_pair_workspace_bytes(int64_t pairs, int64_t K);
int pats_topk_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                          int64_t pairs, int64_t cap, int64_t K, int use_min_conf, float min_conf, float* top_l, float* top_r,
                          float* top_conf, int32_t* top_idx, int64_t* top_count, void* workspace, size_t workspace_bytes,
                          pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair spread top-K (ABI 8, symbols added): the sibling of the per-pair top-K that spreads the selection over the image.  A
 * grid of square cells lies over the points of ONE side; every cell keeps its most confident eligible match, and the K most
 * confident of these winners are the pair's selection, left in the form of the per-pair top-K: whatever reads that result reads
 * this one.  Exact and deterministic, ONE launch for the whole batch, no host read.
 * For pair p let lo, hi, n and i be as in "Per-pair top-K", and key(i) and eligible exactly as defined there.  Further arguments:
 *   side         0 = cells over matches_l, 1 = cells over matches_r
 *   cell         an integer number of pixels, 1 .. 65536
 *   grid0, grid1 cells along component 0 and component 1 of the stored (c0, c1) points; both >= 1 and grid0 * grid1 <= max_cells
 * Definition
 *   u_a(i)     component a of the point of match i on the chosen side (float32)
 *   q_a(i)     u_a > 0 ? (int)min(u_a, 16777216.0f) : 0: a NaN, a negative value and -inf give 0, +inf gives 2^24; the floor of a
 *              float, exact
 *   c_a(i)     min(q_a / cell, grid_a - 1): integer division; a point outside the grid falls into the edge cell
 *   cellid(i)  c_0 * grid1 + c_1
 *   winner(g)  among the ELIGIBLE matches with cellid == g: the largest key, ties by the lowest i; a cell without an eligible match
 *              has none
 *   ranking    the winners by key descending, ties by i ascending
 *   occupied   [pairs] int64: the number of winners (cells with at least one eligible match)
 *   top_count  [pairs] int64: min(K, occupied)
 *   top_l, top_r, top_conf, top_idx: as in "Per-pair top-K" over that ranking - bit-for-bit copies for j < count, -1 / 0.0 behind it
 * It follows that every call defines every byte of every output; that the result does not depend on any order of execution; that a
 * batch in which no two eligible matches of a pair share a cell returns exactly what pats_topk_by_pair_f32 returns; and that
 * grid0 = grid1 = 1 returns each pair's single best eligible match.  The selection is NOT a subset of the plain top-K.
 * max_cells = pats_topk_spread_by_pair_max_cells() = 16384: the cell table of one pair lives in LDS at 8 bytes per cell (128 KiB
 * of the 160 a workgroup may allocate; a launch asks for what its grid needs, rounded up to a power of two).  With K <= 8192 more
 * cells buy nothing; a caller whose grid is larger takes a larger cell.
 * Refused before any launch (pats_last_error names the argument), in this order: everything pats_topk_by_pair_f32 refuses; occupied
 * null or off 8 bytes; side not 0 or 1; cell outside 1 .. 65536; grid0 < 1; grid1 < 1; grid0 * grid1 > max_cells.  cap == 0 is a
 * valid call.  PATS_ERR_UNSUPPORTED if the device refuses the LDS a grid above 8192 cells needs.  The workspace query answers 0
 * today (workspace may then be null). */
int64_t pats_topk_spread_by_pair_max_cells(void);
size_t pats_topk_spread_by_pair_workspace_bytes(int64_t pairs, int64_t K, int64_t grid0, int64_t grid1);
int pats_topk_spread_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                 int64_t pairs, int64_t cap, int64_t K, int use_min_conf, float min_conf, int side, int64_t cell,
                                 int64_t grid0, int64_t grid1, float* top_l, float* top_r, float* top_conf, int32_t* top_idx,
                                 int64_t* top_count, int64_t* occupied, void* workspace, size_t workspace_bytes,
                                 pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair model verification (ABI 8, symbols added): H candidate epipolar models per pair tested against every match of the
 * pair, the model with the most inliers, its inlier mask and - on request - the moment matrix of its inliers.  The O(H M) step
 * of a hypothesise-and-verify search on the hand-over (or on a per-pair top-K of it), on the device, no host read; everything
 * after the mask (cheirality, pose) is pats_epipolar_pose_by_pair_f64 below, and the hypotheses are the caller's own or those of
 * pats_epipolar_hypotheses_by_pair_f32.
 * Inputs
 *   matches_l, matches_r [cap,2] float32, the stored (c0, c1) of the hand-over taken as they lie; conf [cap] float32 (optional)
 *   the segment of pair p, in exactly ONE of two forms (both or neither: refused)
 *     ragged   pair_off: int64, pairs + 1 entries (a longer buffer that starts with them - the summary buffer - is fine):
 *              lo = pair_off[p], hi = pair_off[p + 1], both clamped to [0, cap] on the device, hi <= lo is an empty pair: a stale
 *              table never causes a read outside the arrays.  (Where the segments of a corrupt table overlap, a row's mask is
 *              that of one of its pairs.)  stride is ignored.
 *     strided  counts_in [pairs] int64 and stride (the layout of the top-K outputs top_l / top_r / top_count): the segment starts
 *              at p * stride and holds min(max(counts_in[p], 0), stride) rows; cap >= pairs * stride
 *   models [pairs,H,3,3] float32, contiguous, row-major E; 1 <= H <= pats_epipolar_max_h() (65536: what the grid of the score
 *              kernel and an int32 index carry comfortably; the kernel itself walks the models in chunks of 256)
 *   thr [pairs] float32.  It lives on the device and cannot be refused: a pair whose thr is NaN or negative has NO inliers
 *              (counts 0, best 0, best_count 0, mask 0, moments 0); the other pairs are unaffected
 *   norm [pairs,8] float32 (optional) = (c0_l, c1_l, s0_l, s1_l, c0_r, c1_r, s0_r, s1_r): a point p becomes
 *              x = ((p0 - c0) * s0, (p1 - c1) * s1, 1) - in float32 one subtract, then one multiply, never contracted, so a host
 *              reproduces x bit for bit.  Without norm x = (p0, p1, 1)
 *   use_min_conf, min_conf: a match PARTICIPATES iff use_min_conf == 0 or conf >= min_conf (inclusive; a NaN confidence does not
 *              participate) - and iff its four coordinates, after norm, are finite
 * The test of match i against model E:
 *   a = E x_l,  b = E^T x_r,  r = x_r . a,  den = a0^2 + a1^2 + b0^2 + b1^2
 *   inlier iff the match participates and den > 0 and r^2 <= thr^2 den
 * - the squared Sampson error against thr^2 without the division.  A NaN anywhere makes it a non-inlier; an all-zero model has
 * den = 0 and so no inliers: zero models may pad H.  The device evaluates it in float32 with fused multiply-adds (a0 =
 * fma(E00, x0, fma(E01, x1, E02)), ..., den = fma(a0, a0, fma(a1, a1, fma(b0, b0, b1 b1)))); a verdict whose r^2 lies within a few
 * float32 roundings of thr^2 den may differ from a float64 evaluation (docs/parity.md quantifies the band), but the counts, the
 * winner and the mask of one call always agree with each other: one arithmetic serves all three.
 * Outputs - every call defines every byte of every output
 *   counts [pairs,H] int32      the inliers of every model
 *   best [pairs] int32          the lowest index with the largest count;  best_count [pairs] int64 that count
 *   inlier [cap] uint8          aligned with the input lists: 1 where the match is an inlier of its pair's best model, 0 everywhere
 *                               else - rows outside every segment and the slack of strided rows included
 *   moments [pairs,9,9] float64 (null: skipped) sum over the best model's inliers of q q^T, q = vec(x_r x_l^T) - the nine products
 *                               in row-major order, formed in float64 from the float32 x (exact).  The summation order is fixed:
 *                               two calls are bit-identical.  The eigenvector of the smallest eigenvalue is the least-squares refit
 * cap == 0 is a valid call (counts 0, outputs defined; the match pointers must still be non-null).  Refused before any launch
 * (pats_last_error names the argument): a null matches_l / matches_r / models / thr / counts / best / best_count / inlier;
 * matches_l / matches_r off 8 bytes (read as float2), models / thr / norm / conf / counts / best off 4, pair_off / counts_in /
 * best_count / moments off 8; both segment forms or neither; pairs < 1; H < 1 or H > max_h; cap < 0 or cap >= 2^31 - 1; in the strided
 * form stride < 1 or pairs * stride > cap; use_min_conf without conf or with a NaN or negative min_conf; a grid of 2^31 workgroups
 * or more (ceil(longest / 2048) * pairs * ceil(H / 256), longest = cap or stride); a workspace smaller than
 * pats_epipolar_workspace_bytes (0 today: the counts are accumulated in the output; workspace may then be null). */
int64_t pats_epipolar_max_h(void);
size_t pats_epipolar_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_epipolar_score_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                    int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                    int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                    int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                    void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair hypotheses (ABI 8, symbols added): the H candidate models pats_epipolar_score_by_pair_f32 tests, generated on the
 * device - for every pair p and every h in 0 .. H-1 eight distinct matches of the pair are drawn and the unit null vector of their
 * 8x9 epipolar constraint matrix (the 8-point algorithm's linear step) is written as a row-major 3x3 model.  One launch, no host
 * read, deterministic: the draws come from a counter-based generator that a host reproduces exactly.  Not here: a 7-point solver
 * (the 5-point one is pats_epipolar_hypotheses5_by_pair_f32 below), the rank-2 / essential projection of a hypothesis, cheirality and
 * pose, local optimisation (pats_epipolar_polish_by_pair_f32 below), adaptive termination.
 * Inputs
 *   matches_l, matches_r [cap,2] float32 and the segment of pair p - ragged (pair_off) or strided (stride, counts_in), exactly ONE
 *              of the two forms (both or neither: refused) - as for pats_epipolar_score_by_pair_f32, with the same clamping:
 *              ragged   lo = pair_off[p], hi = pair_off[p + 1], both clamped to [0, cap] on the device, hi <= lo is an empty pair
 *              strided  the segment starts at p * stride and holds min(max(counts_in[p], 0), stride) rows; cap >= pairs * stride
 *              n = the pair's count, lo = its first row
 *   norm [pairs,8] float32 (optional): x = ((p0 - c0) * s0, (p1 - c1) * s1, 1), the verification's rule - in float32 one subtract,
 *              then one multiply, never contracted.  Without norm x = (p0, p1, 1)
 *   pair_seed [pairs] int64, on the device; progressive: 0 or 1; 1 <= H <= pats_epipolar_max_h()
 * The pool of hypothesis h: m_h = n for progressive == 0, otherwise m_h = max(8, (n (h + 1) + H - 1) / H) in int64 arithmetic - on a
 * list sorted by confidence (a per-pair top-K) the early hypotheses draw from the most confident matches, the last one from all.
 * The sampler - all arithmetic uint32, wrapping:
 *   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   s_lo, s_hi = the low and the high 32 bits of pair_seed[p];  k = mix(mix(mix(s_lo) ^ s_hi) + h)
 *   u_t = mix(k + 0x9e3779b9 * (t + 1)),  j_t = (uint64(u_t) * (m_h - t)) >> 32          for t = 0 .. 7
 *   draw t is the j_t-th index (from 0) of 0 .. m_h - 1 that no earlier draw took - equivalently: walk the earlier draws in ascending
 *   order and add 1 to j for each one that is <= j.  sample_idx[p,h,t] is that position inside the pair's list, in draw order.
 * The eight indices are distinct and < m_h; there is no rejection loop.
 * The model: A [8,9] has row t = vec(x_r x_l^T) of draw t - q[3i + j] = x_r[i] x_l[j], the q of `moments` above.  models[p,h] is a
 * float32 vector e with A e = 0 and Frobenius norm 1, its sign such that the component of largest magnitude is positive (the lowest
 * index among equals, judged on the values written).  No component is pinned: a null vector with e[8] = 0 (a sideways translation)
 * is found like any other.
 * The ZERO model - nine exact zeros, the padding the verification ignores - is written
 *   for every h of a pair with n < 8; sample_idx is then -1 for every h and t
 *   for a sample one of whose 32 coordinates is not finite after norm; sample_idx is still written
 *   for a sample whose solve does not end finite (coordinates whose squares leave the float32 range)
 * A rank-deficient sample (duplicated matches, ...) gives the zero model or a finite unit vector of the null space, never a NaN or
 * an infinity.
 * Accuracy: the solve is float32.  The contract is a backward error, not an algorithm: with the written e promoted to float64 and
 * A formed exactly from the float32 x,  |A e|_2 <= B eps32 |A|_F  and  | |e| - 1 | <= 1e-5  for every nonzero model; the tests hold B
 * to 8 times what LAPACK's float32 SVD reaches on the same samples (docs/parity.md has the measured values).
 * Outputs - every call defines every byte of both
 *   models [pairs,H,3,3] float32;  sample_idx [pairs,H,8] int32 (optional: null skips it)
 * cap == 0 is a valid call (every model zero; the match pointers must still be non-null).  Refused before any launch
 * (pats_last_error names the argument): a null matches_l / matches_r / pair_seed / models; matches_l / matches_r off 8 bytes (read
 * as float2), models / norm / sample_idx off 4, pair_off / counts_in / pair_seed off 8; both segment forms or neither; pairs < 1;
 * H < 1 or H > max_h; cap < 0 or cap >= 2^31 - 1; in the strided form stride < 1 or pairs * stride > cap; progressive not 0 or 1;
 * a grid of 2^31 workgroups or more (pairs * ceil(H / 64)); a workspace smaller than pats_epipolar_hypotheses_workspace_bytes
 * (0 today: a hypothesis lives in its thread's registers; workspace may then be null). */
size_t pats_epipolar_hypotheses_workspace_bytes(int64_t pairs, int64_t H);
int pats_epipolar_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                         const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                         const float* norm, int progressive, float* models, int32_t* sample_idx, void* workspace,
                                         size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair 5-point hypotheses (ABI 8, symbols added): the calibrated sibling of the per-pair hypotheses above - for every pair p and
 * every sample h in 0 .. H-1 FIVE distinct matches of the pair are drawn and the real essential matrices through them, at most ten,
 * are written as row-major 3x3 models.  What cv2.findEssentialMat's RANSAC solves per sample.  One launch, no host read, no
 * workspace, deterministic.  The points must be calibrated: norm carries the intrinsics ((c, s) = (principal point, 1 / focal
 * length) per side); without norm the solver runs on (p0, p1, 1) as if those were calibrated coordinates.
 * What it is not: cheirality and pose (pats_epipolar_pose_by_pair_f64), local optimisation (pats_epipolar_polish_by_pair_f32),
 * adaptive termination; the uncalibrated sibling is pats_epipolar_hypotheses7_by_pair_f32.
 *   x          the verification's point, formed exactly as there: ((p0 - c0) * s0, (p1 - c1) * s1, 1) in float32 - one subtract,
 *              then one multiply, never contracted - or (p0, p1, 1) without norm.  The segment of pair p (n rows from lo on) in the
 *              same two forms, ragged (pair_off) or strided (stride, counts_in), with the same clamping as above
 *   pool       m_h = n (progressive == 0)  or  max(5, (n (h + 1) + H - 1) / H)  in int64 arithmetic
 *   sampler    the one above with five draws: k = mix(mix(mix(s_lo) ^ s_hi) + h),  u_t = mix(k + 0x9e3779b9 (t + 1)),
 *              j_t = (uint64(u_t) (m_h - t)) >> 32,  t = 0 .. 4,  draw t = the j_t-th index of 0 .. m_h - 1 not drawn before
 *   sample_idx [pairs,H,5] int32 (optional: null skips it), the draws in draw order;  -1 for n < 5
 *   solutions  A5 [5,9], row t = vec(x_r x_l^T) of draw t (q[3i + j] = x_r[i] x_l[j]).  A solution is a 3x3 E, |E|_F = 1, with
 *              A5 vec(E) = 0 and 2 E E^T E - tr(E E^T) E = 0 (hence det E = 0): the real essential matrices through the five
 *              matches, at most 10
 *   models     [pairs,H,10,3,3] float32, row-major.  The solutions found occupy the lowest slots of their sample, every other slot
 *              is nine exact zeros.  Each non-zero model has the component of largest magnitude positive (the lowest index among
 *              equals, judged on the values written: the hypotheses' convention).  The non-zero models of a sample are pairwise
 *              distinct, 1 - |<a, b>| > 1e-6: where two roots lie closer (a sample at the edge between k and k + 2 real
 *              solutions) one model stands for both.  The order among the non-zero slots is unspecified but identical from call to
 *              call.  Viewed as [pairs, 10 H, 3, 3] it is a `models` argument of pats_epipolar_score_by_pair_f32 as it stands
 *   n_models   [pairs,H] int32 (optional: null skips it): the number of non-zero slots
 *   zero       all ten slots zero (n_models 0): n < 5 (sample_idx -1);  a sample with a non-finite coordinate after norm (sample_idx
 *              still written);  a degenerate sample (a pivot of the elimination that is zero or not finite, a polynomial without a
 *              leading term);  a sample without a real solution.  Never a NaN or an infinity
 *   contract   every non-zero model e, promoted to float64, with A5 formed exactly from the float32 points:
 *                | |e| - 1 | <= 1e-5
 *                |A5 e|_2                      <= B_epi eps32 |A5|_F
 *                |2 E E^T E - tr(E E^T) E|_F   <= B_ess eps32
 *              The solve is float64 (null space by Householder QR, Gauss-Jordan with partial pivoting on the ten cubic
 *              constraints, the degree-10 polynomial in z, a Sturm chain, bisection and Newton steps with fixed caps); the kernel
 *              evaluates the third residual itself, in float64 on the float32 values it is about to store, and writes NOTHING for
 *              a root whose residual exceeds 4 eps32 (rounding an exact solution to float32 costs at most 3): an ill-conditioned
 *              root is dropped, never emitted.  So every non-zero model is a solution of the sample's problem to working accuracy;
 *              completeness is a tested share (docs/parity.md), not a pointwise promise.  The tests hold B_epi and B_ess to 8
 *              times what a float64 LAPACK solve, rounded to float32, reaches on the same samples
 *   limits     1 <= H and 10 H <= pats_epipolar_max_h()
 * Outputs - every call defines every byte of all three.  cap == 0 is a valid call (every model zero; the match pointers must still
 * be non-null).  Refused before any launch (pats_last_error names the argument): what pats_epipolar_hypotheses_by_pair_f32 refuses,
 * n_models off 4 bytes, 10 H > max_h (the message names H), a grid of 2^31 workgroups or more (pairs * ceil(H / 64)); a workspace
 * smaller than pats_epipolar_hypotheses5_workspace_bytes (0 today: a sample lives in its thread's registers and 1888 bytes of LDS;
 * workspace may then be null).  PATS_ERR_UNSUPPORTED if the device does not grant a workgroup its 120832 bytes of LDS. */
size_t pats_epipolar_hypotheses5_workspace_bytes(int64_t pairs, int64_t H);
int pats_epipolar_hypotheses5_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                          const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                          const float* norm, int progressive, float* models, int32_t* sample_idx, int32_t* n_models,
                                          void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair relative pose (ABI 8, symbols added): from the inliers pats_epipolar_score_by_pair_f32 marked to (R, t) per pair - the
 * least-squares refit of the winner's moments, its projection onto the essential matrices, the four decompositions and the
 * cheirality vote that picks one.  What findEssentialMat's last step and recoverPose do after a hypothesise-and-verify search, on
 * the device, no host read.  The returned E, cast to float32, is a valid unit model: fed back as an H = 1 model it gives the local-
 * optimisation round (pose -> verify -> moments -> pose).
 * What it is not: there is no distance threshold on the triangulated points (the reference passes 1e9 to recoverPose: effectively
 * none), no minimal solver (the 5-point hypotheses are pats_epipolar_hypotheses5_by_pair_f32 above), no pose-error metric, and
 * nothing in pipeline.forward_* or the drop-in calls it.
 * Inputs
 *   matches_l, matches_r [cap,2] float32, the segment of pair p - ragged (pair_off) or strided (stride, counts_in), exactly ONE of
 *              the two forms - and norm [pairs,8] float32 (optional): as for pats_epipolar_score_by_pair_f32, with the same clamping
 *   inlier [cap] uint8        the mask the verification wrote beside those lists
 *   best_count [pairs] int64  the verification's; a pair with best_count < 8 has no pose
 *   the refit's source: moments [pairs,9,9] float64 (the verification's; the upper triangle is read), or - when moments is null -
 *              models [pairs,H,3,3] float32 with best [pairs] int32 (clamped to 0 .. H-1).  With moments given, models and best
 *              are not read
 *   swapped    0 or 1, see below
 * Definition, per pair
 *   x           the verification's point, formed exactly as there (float32: one subtract, one multiply; (p0, p1, 1) without norm)
 *   used        inlier[i] != 0 and the four coordinates of x finite
 *   e_refit     [pairs,9] float64 (optional output).  With moments: a unit eigenvector of moments[p] for its smallest eigenvalue
 *               (float64 throughout; the lowest index among equal eigenvalues, either sign).  Without: models[p, best[p]] promoted
 *               to float64.  Nine zeros for a pair without a pose because of best_count or a non-finite value
 *   E           [pairs,3,3] float64: the essential matrix nearest to e_refit, E = U diag(s, s, 0) V^T from e_refit =
 *               U diag(s1, s2, s3) V^T, rescaled to Frobenius norm 1 (s = 1/sqrt 2).  The component of largest magnitude is positive
 *               (the lowest index among equals): the hypotheses' convention.  Cast to float32 it is a valid model for
 *               pats_epipolar_score_by_pair_f32
 *   candidates  det U, det V > 0;  W = [[0,-1,0],[1,0,0],[0,0,1]];  R1 = U W V^T,  R2 = U W^T V^T,  u = U[:,2]
 *               order: (R1, u), (R2, u), (R1, -u), (R2, -u).  (The SVD leaves U and V free up to a joint rotation of the first two
 *               columns and joint signs; the SET of four is unique, which of its members is R1 is not.)
 *               convention: x_r ~ R x_l + t, so E ~ [t]x R - OpenCV's
 *   in front    for a used match and candidate (R, t), with R and t rounded to float32 and float32 arithmetic:
 *                 a = R x_l,  b = x_r,  c = a x b
 *                 in front  iff  c.c > 0  and  c.(b x t) > 0  and  c.(a x t) > 0
 *               - the signs of the two depths of the least-squares intersection of the rays, without a division:
 *                 lambda_l = c.(b x t) / c.c,   lambda_r = c.(a x t) / c.c
 *               A verdict whose dot product lies within a few float32 roundings of zero may differ from a float64 evaluation
 *               (docs/parity.md quantifies the band); the counts, the choice and the mask of one call always agree: one device
 *               function serves all three
 *   no pose     best_count[p] < 8, a non-finite moment or e_refit, or s2 == 0 (e_refit of rank below 2):
 *               E = 0, R = I, t = 0, all counts 0, choice 0, front 0.  Never a NaN or an infinity in any output
 *   swapped     with 1 the points are in the hand-over's (c0, c1) = (y, x) order.  Everything is computed in that frame and written
 *               in the reference's:  R_out = P R P,  t_out = P t,  E_out = P E P (sign rule applied after the permutation),
 *               P = [[0,1,0],[1,0,0],[0,0,1]] - X' = P X turns X_r = R X_l + t into X_r' = (P R P) X_l' + P t with the depths
 *               unchanged.  front_counts, choice and front do not depend on it; e_refit stays in the input frame
 * Outputs - every call defines every byte of every output
 *   E [pairs,3,3], R [pairs,3,3], t [pairs,3] float64: the chosen candidate, |t| = 1
 *   front_counts [pairs,4] int32   used matches in front, per candidate
 *   choice [pairs] int32           the lowest candidate index with the largest count;  front_count [pairs] int64 that count
 *   front [cap] uint8 (optional)   1 where a used match is in front under the chosen candidate, 0 everywhere else - rows outside
 *                                  every segment and the slack of strided rows included.  Its sum over a segment is front_count
 *   e_refit [pairs,9] float64 (optional)
 * cap == 0 is a valid call that defines every per-pair output (the match pointers and inlier must still be non-null).  Refused
 * before any launch (pats_last_error names the argument): a null matches_l / matches_r / inlier / best_count / E / R / t /
 * front_counts / choice / front_count; matches_l / matches_r off 8 bytes (read as float2), moments / E / R / t / e_refit / pair_off /
 * counts_in / best_count / front_count off 8, models / best / norm / front_counts / choice off 4; both segment forms or neither;
 * pairs < 1; cap < 0 or cap >= 2^31 - 1; in the strided form stride < 1 or pairs * stride > cap; swapped not 0 or 1; neither moments
 * nor (models and best); with models given H < 1 or H > max_h; a workspace smaller than
 * pats_epipolar_pose_workspace_bytes (0 today: the solve lives in LDS and registers; workspace may then be null). */
size_t pats_epipolar_pose_workspace_bytes(int64_t pairs, int64_t cap);
int pats_epipolar_pose_by_pair_f64(const float* matches_l, const float* matches_r, const uint8_t* inlier, const int64_t* pair_off,
                                   int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const int64_t* best_count,
                                   const double* moments, const float* models, int64_t H, const int32_t* best, const float* norm,
                                   int swapped, double* E, double* R, double* t, int32_t* front_counts, int32_t* choice,
                                   int64_t* front_count, uint8_t* front, double* e_refit, void* workspace, size_t workspace_bytes,
                                   pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair triangulation (ABI 8, symbols added): from a pair's pose and a mask over its matches to 3-D points - for every masked
 * match the midpoint of the common perpendicular of its two rays, the two depths, the squared reprojection error and the cosine of
 * the triangulation angle, and per pair the number of valid points and the sum of their errors.  What two-view initialisation,
 * keyframe selection, depth seeding and a filter by reprojection error or parallax start from, on the device, no host read.
 * What it is not: the optimal (Hartley-Sturm) correction - this is the midpoint; no bundle adjustment; the scale is the baseline's
 * (|t| = 1); calibrated coordinates only (the uncalibrated branch, pats_fundamental_refit_by_pair_f64, has no triangulation); and
 * nothing in pipeline.forward_* or the drop-in calls it.
 * Inputs
 *   matches_l, matches_r [cap,2] float32, the segment of pair p - ragged (pair_off) or strided (stride, counts_in), exactly ONE of
 *              the two forms - and norm [pairs,8] float32 (optional): as for pats_epipolar_score_by_pair_f32, with the same clamping
 *   mask [cap] uint8          aligned with the lists: the pose's front, or the verification's inlier
 *   R [pairs,3,3], t [pairs,3] float64, as pats_epipolar_pose_by_pair_f64 wrote them (with the same swapped)
 *   swapped    0 or 1: what pats_epipolar_pose_by_pair_f64 was given
 *   max_reproj [pairs] float32 (optional), max_cos [pairs] float32 (optional): the limits below
 * Definition, per match i of pair p
 *   x          the verification's point, formed exactly as there (float32: one subtract, one multiply; (p0, p1, 1) without norm);
 *              then promoted to float64
 *   used       mask[i] != 0 and the four coordinates of x finite
 *   R_p, t_p   swapped ? (P R P, P t) : (R, t),  P = [[0,1,0],[1,0,0],[0,0,1]] - the pose in the frame of the points; float64, NOT
 *              rounded to float32.  A pair with a non-finite entry in R or t, or t = 0 (the pose's "no pose"), has no valid match
 *   a = R_p x_l,  b = x_r = (r0, r1, 1),  c = a x b,  cc = c.c
 *   lambda = c.(b x t_p) / cc,   mu = c.(a x t_p) / cc     the depths in the left / right camera (x has third component 1)
 *   X_r = (lambda a + t_p + mu b) / 2                      the midpoint of the common perpendicular, right camera frame
 *   X   = R_p^T (X_r - t_p)                                the same point in the LEFT camera frame: the output frame
 *   e2  = |pi(X) - x_l|^2 + |pi(R_p X + t_p) - x_r|^2,  pi(v) = (v0 / v2, v1 / v2)    squared reprojection error, the points' units
 *   cosp = a.b / (|a| |b|)                                 cosine of the triangulation angle
 *   valid      used and cc > 0 and lambda > 0 and mu > 0 and X[2] > 0 and (R_p X + t_p)[2] > 0 and every value above finite -
 *              X, lambda, mu, e2 and cosp of magnitude at most FLT_MAX, so that their float32 roundings are finite too -
 *              and (max_reproj null or e2 <= (double)max_reproj[p]^2) and (max_cos null or cosp <= (double)max_cos[p])
 *              (a NaN limit makes every comparison false: nothing valid)
 * All arithmetic after the point is formed is float64, no contraction, in this order (sums left to right, brackets first):
 *   a_i = (R_p[i,0] l0 + R_p[i,1] l1) + R_p[i,2];  the cross products by components, u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2,
 *   u0 v1 - u1 v0) with b2 = 1 not multiplied;  every dot product (u0 v0 + u1 v1) + u2 v2;  X_r - t_p by components as
 *   ((lambda a_i + t_i) + mu b_i) * 0.5 - t_i;  X_j = (R_p[0,j] q0 + R_p[1,j] q1) + R_p[2,j] q2;  (R_p X + t_p)_i =
 *   ((R_p[i,0] X0 + R_p[i,1] X1) + R_p[i,2] X2) + t_i;  e2 = (d0^2 + d1^2) + (d2^2 + d3^2), left differences first;
 *   cosp = a.b / (sqrt(a.a) sqrt(b.b)).  A float64 restatement that orders them differently agrees far below a float32 step.
 * Outputs - every call defines every byte of every output; a row that is not valid (not used, in no segment, the slack of a strided
 * row, behind a camera, over a limit, degenerate) holds exact zeros in every per-match output.  Never a NaN or an infinity
 *   points [cap,3] float32          X rounded once; with swapped = 1 in the reference's frame (P X: the first two components exchanged)
 *   depths [cap,2] float32 (optional)   (lambda, mu)
 *   reproj [cap] float32 (optional)     e2
 *   cos_parallax [cap] float32 (optional)   cosp
 *   valid [cap] uint8               1 where the match is valid, else 0
 *   tri_count [pairs] int64         the valid matches of the pair: valid's sum over the segment, exactly
 *   reproj_sum [pairs] float64      the sum of e2 (float64, before the rounding) over the pair's valid matches, added in an order the
 *                                   sizes alone fix: two calls give the same bits
 * cap == 0 is a valid call that defines every per-pair output (the match pointers, mask, points and valid must still be non-null).
 * Refused before any launch (pats_last_error names the argument): a null matches_l / matches_r / mask / R / t / points / valid /
 * tri_count / reproj_sum; matches_l / matches_r off 8 bytes (read as float2), R / t / tri_count / reproj_sum / pair_off / counts_in
 * off 8, norm / max_reproj / max_cos / points / depths / reproj / cos_parallax off 4; both segment forms or neither; pairs < 1;
 * cap < 0 or cap >= 2^31 - 1; in the strided form stride < 1 or pairs * stride > cap; swapped not 0 or 1; a workspace smaller than
 * pats_epipolar_triangulate_workspace_bytes (0 today: everything lives in LDS and registers; workspace may then be null). */
size_t pats_epipolar_triangulate_workspace_bytes(int64_t pairs, int64_t cap);
int pats_epipolar_triangulate_by_pair_f64(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                          const int64_t* counts_in, int64_t pairs, int64_t cap, const uint8_t* mask, const float* norm,
                                          const double* R, const double* t, int swapped, const float* max_reproj, const float* max_cos,
                                          float* points, float* depths, float* reproj, float* cos_parallax, uint8_t* valid,
                                          int64_t* tri_count, double* reproj_sum, void* workspace, size_t workspace_bytes,
                                          pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair pose error and AUC (ABI 8, symbols added): what the reference's evaluation does with a pose - the rotation error and the
 * translation error of every pair against the ground truth (utils/metrics.py:56-66: angle_error_mat, angle_error_vec and the fold of
 * the translation angle at 90 degrees), and the AUC of the recall curve over a data set's worth of them (metrics.py:70-96: error_auc
 * under aggregate_metrics) - on the device, no host read.  What it is not: an estimator (the pose comes from
 * pats_epipolar_pose_by_pair_f64); a match-precision metric (pats_match_error_by_pair_f64 is that; the verification with the ground
 * truth's essential matrix as the one model is its epipolar form); and nothing in pipeline.forward_*, the drop-in or bench.py calls it.
 *
 * pats_pose_error_by_pair_f64 - one launch for the batch, float64 throughout
 * Inputs
 *   R [pairs,3,3], t [pairs,3] float64   the estimate, as pats_epipolar_pose_by_pair_f64 wrote it.  Estimate and ground truth must be
 *              in the SAME frame - there is no swapped here: with the data set's extrinsics as the ground truth the pose stage is
 *              called with swapped = 1 (the reference's (x, y) frame)
 *   T1 [pairs,4,4] float64, row-major    only the upper 3 x 4 is read: (R1 | t1)
 *   T0 [pairs,4,4] float64 (optional)    only the upper 3 x 4 is read: (R0 | t0)
 *   counts [pairs] int64 (optional)      the pair's number of matches (the reference's kp1.shape[0])
 *   min_matches  the reference's 15;  min_gt_t >= 0, 0 for the reference's behaviour wherever that is defined
 * Definition, per pair p (float64, no contraction, sums left to right, brackets first)
 *   ground truth   without T0: R_gt = R1, t_gt = t1.  With T0 the rigid form of the reference's T1 inv(T0):
 *              R_gt[i][j] = (R1[i][0] R0[j][0] + R1[i][1] R0[j][1]) + R1[i][2] R0[j][2]                    (R1 R0^T)
 *              t_gt[i] = t1[i] - ((R_gt[i][0] t0[0] + R_gt[i][1] t0[1]) + R_gt[i][2] t0[2])
 *              The reference inverts T0 by a general LU factorisation: for a rigid T0 the two differ by rounding only
 *   err_R      s = R[0][0] R_gt[0][0], then s = s + R[i][j] R_gt[i][j] for the other eight entries in row-major order;
 *              c = (s - 1) / 2, clipped to [-1, 1];  err_R = acos(c) * 57.29577951308232 (180 / pi)       angle_error_mat
 *   err_t      d = (t[0] t_gt[0] + t[1] t_gt[1]) + t[2] t_gt[2];  |v| = sqrt((v[0]^2 + v[1]^2) + v[2]^2);  c = d / (|t| |t_gt|),
 *              clipped;  e = acos(c) * 57.29577951308232;  err_t = min(e, 180 - e)      angle_error_vec and the fold of metrics.py:63
 *              If |t_gt| <= min_gt_t the direction of t_gt carries no information and err_t = 0 - a stated departure: for t_gt = 0
 *              the reference produces a NaN
 *   err        max(err_R, err_t): what aggregate_metrics feeds the AUC
 *   status     the lowest number that applies:
 *              0 evaluated;  1 counts given and counts[p] < min_matches;  2 no pose: an entry of R or t that is not finite, or
 *              t = 0 (pats_epipolar_pose_by_pair_f64's "no pose");  3 an entry that is not finite in the ground truth that was read
 *              (the upper 3 x 4 of T1, and of T0 if given)
 *   For status != 0 all three errors are +inf: the reference's value for a pair it cannot score.  A NaN that arises in the
 *   arithmetic of an evaluated pair (an overflow of finite inputs) is written as +inf as well.  Unlike every other stage of this
 *   library +inf is therefore a legitimate VALUE of these outputs; a NaN never is.
 * Outputs - every call defines every byte
 *   err_R, err_t, err [pairs] float64 (degrees), status [pairs] int32
 * Refused before the launch (pats_last_error names the argument): a null R / t / T1 / err_R / err_t / err / status; R / t / T1 / T0 /
 * counts / err_R / err_t / err off 8 bytes, status off 4; pairs < 1; min_matches < 0; min_gt_t negative or a NaN.
 *
 * pats_pose_auc_f64 - one workgroup, one launch
 * Inputs
 *   errors [n] float64 on the device, 0 <= n <= pats_pose_auc_max_n() (16384: the keys live in LDS); a NaN counts as +inf and
 *              -0.0 as +0.0 (the stage above never writes either)
 *   thresholds   n_thr HOST doubles, 1 <= n_thr <= 8, each finite and > 0 (the reference's are 5, 10, 20)
 * Definition, per threshold thr
 *   e_(1) <= ... <= e_(n)   the errors sorted ascending (as order-preserving 64-bit keys, bitonic; equal keys are equal values)
 *   k = the number of errors STRICTLY below thr (searchsorted's left side: an error equal to the threshold is out)
 *   x_0 = 0, x_i = e_(i);  y_i = i * (1 / n)
 *   area = sum over i < k of ((x_{i+1} - x_i) * (y_i + y_{i+1})) * 0.5, plus (thr - x_k) * y_k;  auc = area / thr
 *   This is error_auc's np.trapz over [0] + sorted(errors) with the recall np.linspace(0, 1, n + 1), cut at thr (the reference
 *   ignores its thresholds argument and always uses 5, 10, 20; this function uses what it is given).  n = 0: auc = 0, below = 0.
 *   The sum runs in an order n alone fixes - thread j of 1024 adds the terms j, j + 1024, ... in that order, lane l of a wave then
 *   takes lane l + 32, + 16, ... + 1, the sixteen waves are added in index order, then the last term - so two calls give the same bits.
 * Outputs
 *   auc [n_thr] float64, below [n_thr] int64 (k), sorted [n] float64 (optional): the sorted list, NaN replaced by +inf and
 *   -0.0 by +0.0
 * Refused before the launch: a null errors / thresholds / auc / below (errors also for n = 0); errors / auc / below / sorted off 8
 * bytes; n < 0 or n > pats_pose_auc_max_n(); n_thr < 1 or > 8; a threshold that is not finite and positive. */
int pats_pose_error_by_pair_f64(const double* R, const double* t, const double* T1, const double* T0, const int64_t* counts,
                                int64_t pairs, int64_t min_matches, double min_gt_t, double* err_R, double* err_t, double* err,
                                int32_t* status, pats_stream_t stream);
int64_t pats_pose_auc_max_n(void);
int pats_pose_auc_f64(const double* errors, int64_t n, const double* thresholds, int64_t n_thr, double* auc, int64_t* below,
                      double* sorted, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair homographies (ABI 8, symbols added): the planar sibling of the three epipolar stages above - 4-point hypotheses, their
 * verification and the least-squares refit of the winner - for pairs whose geometry no epipolar model describes (a wall, a floor or a
 * facade filling both images; a camera that mostly rotates) and for callers without intrinsics who want to align two views.  All on
 * the device, no host read.  A caller runs both branches on the same lists and compares the two best_count; the choice is the
 * caller's.
 * What it is not: no symmetric or backward transfer error (the test is the forward one), no orientation test on a2, no adaptive
 * termination, and nothing in pipeline.forward_* or the drop-in calls it.  The decomposition of H into (R, t, n) and the decision
 * between E and H are "Per-pair pose from a homography and the E-or-H decision" below.
 * Shared by the three entry points, per pair p with the n rows of its segment from lo on:
 *   segment     ragged (pair_off) or strided (stride, counts_in), exactly ONE of the two forms, with the clamping of
 *               pats_epipolar_score_by_pair_f32;  norm [pairs,8] float32 (optional) as there
 *   x           the verification's point, formed exactly as there: ((p0 - c0) * s0, (p1 - c1) * s1, 1) in float32 - one subtract, then
 *               one multiply, never contracted - or (p0, p1, 1) without norm;  r = (r0, r1) the first two coordinates of x_r
 *   model       a row-major 3x3 H with x_r ~ H x_l, |H|_F = 1, the component of largest magnitude positive (the lowest index among
 *               equals, judged on the values written).  Nine exact zeros pad H and score nothing
 *   rows        of match i, for h = vec(H):  A_i = [ -x_l^T, 0 0 0, r0 x_l^T ],  B_i = [ 0 0 0, -x_l^T, r1 x_l^T ]   (A_i h = r0 a2 - a0,
 *               B_i h = r1 a2 - a1 with a = H x_l)
 *
 * 1. Hypotheses: pats_homography_hypotheses_by_pair_f32 - the arguments, in order and meaning, of
 *    pats_epipolar_hypotheses_by_pair_f32.  For every pair and every h in 0 .. H-1 FOUR distinct matches are drawn by the sampler
 *    defined there with four draws: k = mix(mix(mix(s_lo) ^ s_hi) + h),  u_t = mix(k + 0x9e3779b9 (t + 1)),
 *    j_t = (uint64(u_t) (m_h - t)) >> 32,  t = 0 .. 3,  draw t = the j_t-th index of 0 .. m_h - 1 not drawn before;
 *    pool m_h = n (progressive == 0) or max(4, (n (h + 1) + H - 1) / H) in int64 arithmetic.
 *      sample_idx [pairs,H,4] int32 (optional: null skips it), the draws in draw order;  -1 for n < 4
 *      models     [pairs,H,3,3] float32: the unit null vector of the 8x9 matrix A whose rows 2t and 2t + 1 are A_i and B_i of draw t
 *      zero       the zero model is written for every h of a pair with n < 4 (sample_idx -1), for a sample one of whose 16
 *                 coordinates is not finite after norm (sample_idx still written) and for a solve that does not end finite.  A rank-
 *                 deficient sample (three collinear points, repeated matches) gives the zero model or a finite unit vector, never
 *                 a NaN or an infinity
 *      contract   the solve is float32 (Householder QR of A^T, one refinement step).  With the written e promoted to float64 and A
 *                 formed exactly from the float32 x:  |A e|_2 <= B eps32 |A|_F  and  | |e| - 1 | <= 1e-5  for every non-zero model; the
 *                 tests hold B to 8 times what LAPACK's float32 SVD reaches on the same samples (docs/parity.md has the values)
 *    Every call defines every byte of both outputs; cap == 0 is a valid call (every model zero; the match pointers must still be
 *    non-null).  Refused before any launch (pats_last_error names the argument): what pats_epipolar_hypotheses_by_pair_f32 refuses,
 *    in the same order and wording; the workspace is pats_homography_hypotheses_workspace_bytes (0 today).
 *
 * 2. Verification: pats_homography_score_by_pair_f32 - the arguments, in order and meaning, of pats_epipolar_score_by_pair_f32
 *    (models [pairs,H,3,3] float32, 1 <= H <= pats_epipolar_max_h(); thr [pairs] float32 on the device; use_min_conf / min_conf and the
 *    finite rule decide whether a match PARTICIPATES exactly as there).  The test of match i against model H:
 *      a = H x_l,   d0 = a0 - r0 a2,   d1 = a1 - r1 a2
 *      inlier iff the match participates and a2^2 > 0 and d0^2 + d1^2 <= thr[p]^2 a2^2
 *    - the squared forward transfer error |r - a / a2|^2 against thr^2 without the division.  A NaN anywhere makes it a non-inlier;
 *    an all-zero model has a2 = 0 and so no inliers.  The device evaluates it in float32 with fused multiply-adds:
 *      a0 = fma(H00, l0, fma(H01, l1, H02)), a1 and a2 alike;  d0 = fma(-r0, a2, a0);  d1 = fma(-r1, a2, a1);
 *      s = fma(d0, d0, d1 d1);  w = a2 a2;  inlier iff w > 0 and s <= (thr thr) w
 *    A verdict whose s lies within a few float32 roundings of thr^2 a2^2 may differ from a float64 evaluation (docs/parity.md
 *    quantifies the band); the counts, the winner and the mask of one call always agree: one device function serves all three.
 *    Outputs, every byte defined by every call, with the shapes and rules of the epipolar verification:
 *      counts [pairs,H] int32;  best [pairs] int32 (the lowest index of the largest count);  best_count [pairs] int64
 *      inlier [cap] uint8       1 where the match is an inlier of its pair's best model, 0 everywhere else - rows outside every
 *                               segment and the slack of strided rows included.  Its sum over a segment is best_count exactly
 *      moments [pairs,9,9] float64 (null: skipped) the sum over the best model's inliers of A_i^T A_i + B_i^T B_i, the rows formed in
 *                               float64 from the float32 x (exact).  The summation order is fixed: two calls are byte-identical.
 *    A pair whose thr is NaN or negative has NO inliers (counts 0, best 0, best_count 0, mask 0, moments 0).  cap == 0 is a valid
 *    call.  Refused before any launch: what pats_epipolar_score_by_pair_f32 refuses, in the same order and wording; the workspace is
 *    pats_homography_score_workspace_bytes (0 today).
 *
 * 3. Refit: pats_homography_refit_by_pair_f64 - one small launch, float64 throughout.  It reads no match: there is no cap.
 *    Inputs: best_count [pairs] int64 (the verification's); moments [pairs,9,9] float64 (the verification's; the upper triangle is
 *    read) or - when moments is null - models [pairs,H,3,3] float32 with best [pairs] int32 (clamped to 0 .. H-1; with moments given
 *    they are not read); norm [pairs,8] float32 (optional); swapped 0 or 1.
 *      h_refit     a unit eigenvector of moments[p] for its smallest eigenvalue (the lowest index among equal eigenvalues);  without
 *                  moments: models[p, best[p]] promoted to float64 as it is
 *      H           [pairs,3,3] float64 = h_refit, |H|_F = 1 (to float32 accuracy without moments), with the hypotheses' sign rule:
 *                  cast to float32 it is a model for the verification (the local-optimisation round: refit -> verify -> refit)
 *      H_px        [pairs,3,3] float64 (optional: null skips it) = N_r^-1 H N_l rescaled to Frobenius norm 1, same sign rule;
 *                  N = [[s0, 0, -c0 s0], [0, s1, -c1 s1], [0, 0, 1]] per side from norm[p] read as float32 and widened exactly: the
 *                  homography of the stored (c0, c1) coordinates.  Without norm H_px = H
 *      eig         [pairs,2] float64: the two smallest eigenvalues of moments[p], ascending - the caller's degeneracy measure (a
 *                  second one near the first: the inliers do not pin H down);  0, 0 without moments
 *      no model    best_count[p] < 4, a non-finite moment or model, or an all-zero winning model:  H = H_px = 0, eig = 0.  A
 *                  non-finite H_px (a zero scale in norm) is written as zeros on its own.  Never a NaN or an infinity
 *      swapped     with 1 the points are in the hand-over's (c0, c1) = (y, x) order; everything is computed in that frame and H and
 *                  H_px are written as P H P, P = [[0,1,0],[1,0,0],[0,0,1]], the sign rule applied after the permutation
 *    Refused before any launch (pats_last_error names the argument): a null best_count / H_out / eig; best_count / moments / H_out /
 *    H_px / eig off 8 bytes, models / best / norm off 4; pairs < 1; swapped not 0 or 1; neither moments nor (models and best); with models
 *    given H < 1 or H > max_h; a workspace smaller than pats_homography_refit_workspace_bytes (0 today: the solve lives in LDS and
 *    registers; workspace may then be null). */
size_t pats_homography_hypotheses_workspace_bytes(int64_t pairs, int64_t H);
int pats_homography_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                           const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                           const float* norm, int progressive, float* models, int32_t* sample_idx, void* workspace,
                                           size_t workspace_bytes, pats_stream_t stream);
size_t pats_homography_score_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_homography_score_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                      int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                      int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                      int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                      void* workspace, size_t workspace_bytes, pats_stream_t stream);
size_t pats_homography_refit_workspace_bytes(int64_t pairs);
int pats_homography_refit_by_pair_f64(const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                      const int32_t* best, const float* norm, int64_t pairs, int swapped, double* H_out, double* H_px,
                                      double* eig, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair pose from a homography and the E-or-H decision (ABI 8, symbols added): what closes the planar branch the way
 * pats_epipolar_pose_by_pair_f64 closes the epipolar one - the verified homography decomposed into (R, t, n) per pair, the candidate
 * picked by the pair's matches - and the per-pair choice between the two poses, with the chosen branch's masks handed on.  On the
 * device, no host read; the triangulation, the pose error and the AUC take either result as they take the epipolar pose.
 * The decomposition is the eigenvector form of the four-solution algorithm (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision,
 * section 5.3).
 * What it is not: no nonlinear refinement of H or of the pose, no symmetric transfer error, no prior on the normal (the candidates
 * are returned for a caller who has one), calibrated coordinates only, and nothing in pipeline.forward_* or the drop-in calls it.
 *
 * 1. pats_homography_pose_by_pair_f64.  Inputs: matches_l, matches_r, the segment forms with their clamping, norm, the refit's source
 *    (moments, or models + best with H) and swapped exactly as pats_epipolar_pose_by_pair_f64 takes them; inlier [cap] uint8 and
 *    best_count [pairs] int64 are those of pats_homography_score_by_pair_f32; thr [pairs] float32 (optional); min_baseline a double
 *    >= 0.  Definition, per pair; float64 on one thread unless stated otherwise:
 *      x, used     as for the pose stage: the verification's float32 point;  used = inlier[i] != 0 and four finite coordinates
 *      G           h_refit of the homography refit (a unit eigenvector of moments[p] for its smallest eigenvalue, or
 *                  models[p, best[p]] promoted) as a row-major 3x3 in the frame of the points:  x_r ~ G x_l
 *      no pose     best_count[p] < 4, a non-finite moment or h_refit, lambda2 <= 0, (rotation only and l3 <= 0), or a value of the
 *                  decomposition that is not finite (a t_k of length 0 included).  Then R = I, t = n = 0, E = 0, baseline = 0, all
 *                  counts 0, choice 0, status 0, front 0, cand_R = I, cand_t = cand_n = 0.  Never a NaN or an infinity in any output
 *      spectrum    S = G^T G = V diag(lambda1 >= lambda2 >= lambda3) V^T by cyclic Jacobi, v3 = v1 x v2 so det V = +1.
 *                  G' = G / sqrt(lambda2),  l1 = max(lambda1 / lambda2, 1),  l3 = min(max(lambda3 / lambda2, 0), 1)  (the inner
 *                  max: the Jacobi may leave the zero eigenvalue of a singular S a rounding below zero)
 *      sign        workgroup, float32, G' rounded to float32.  For a used match:  a_i = fma(G'_i0, l0, fma(G'_i1, l1, G'_i2)),
 *                  q = fma(r0, a0, fma(r1, a1, a2)) = x_r . (G' x_l);  pos = #(q > 0), neg = #(q < 0);  if neg > pos then G' = -G'
 *      baseline    sqrt(l1) - sqrt(l3): |t| / d of H = R + t n^T / d, the same for all candidates
 *      rotation    l1 - l3 <= 0, or baseline <= min_baseline.  Then R = G' V diag(1/sqrt(l1), 1, 1/sqrt(l3)) V^T, t = n = 0, E = 0,
 *                  status 2, vis[k] = the used count for all k, sup = 0, choice 0, front = used, cand_R = R twice, cand_t = cand_n = 0
 *      candidates  otherwise (status 1), for s = +1 (k = 0) and s = -1 (k = 1):
 *                    u = (sqrt(1 - l3) v1 + s sqrt(l1 - 1) v3) / sqrt(l1 - l3)
 *                    U = [v2, u, v2 x u]     W = [G' v2, G' u, (G' v2) x (G' u)]
 *                    R_k = W U^T             n_k = v2 x u             t_k = (G' - R_k) n_k
 *                  k = 2, 3: (R_0, -t_0, -n_0), (R_1, -t_1, -n_1).  The written t is t_k / |t_k|; cand_t is t_k itself (|t_k| =
 *                  baseline).  Convention x_r ~ R x_l + t, n in the left camera's frame, n . X = d > 0 on the plane.  Which
 *                  member of the set is k = 0 depends on the signs the Jacobi gives v1 and v2 (they permute the four as
 *                  k -> k ^ m, m in 0 .. 3); the SET of four is unique
 *      E_k         [t_k / |t_k|]x R_k scaled to Frobenius norm 1; E is written with the hypotheses' sign rule
 *      vis         workgroup, float32, n_k rounded to float32:  d = fma(n0, l0, fma(n1, l1, n2));  vis[k] = # used matches with d > 0
 *                  for k = 0, 1 and with d < 0 for k = 2, 3 (one dot product serves two candidates)
 *      sup         only with thr: over ALL matches of the segment with four finite coordinates, sup[k] = # with the epipolar
 *                  verification's test (pats_epipolar_score_by_pair_f32) of float32(E_k) against thr[p]^2: w > 0 and s <= lim;
 *                  sup[2] = sup[0], sup[3] = sup[1].  A NaN or negative thr gives 0.  Without thr: 0
 *      choice      the lowest k with the lexicographically largest (vis[k], sup[k]);  front_count = vis[choice].  Two candidates
 *                  often see every plane point in front - the known two-fold ambiguity; the matches off the plane decide through sup
 *      front       [cap] uint8, optional: 1 where a used match is on the visible side of n_choice, 0 everywhere else.  Every byte is
 *                  written; its sum over a segment is front_count exactly (one device function serves the counts and the mask)
 *      swapped     as in the pose stage:  R -> P R P,  t -> P t,  n -> P n,  E -> P E P (sign rule after the permutation), the
 *                  candidates alike;  vis, sup, choice, status, baseline and front do not depend on it
 *    A float32 verdict within a few roundings of zero (sign, vis) or of the limit (sup) may differ from a float64 evaluation;
 *    docs/parity.md quantifies the band.
 *    Outputs - every call defines every byte of every output:  E, R [pairs,3,3], t, n [pairs,3], baseline [pairs] float64;  vis, sup
 *    [pairs,4], choice, status [pairs] int32;  front_count [pairs] int64;  optional (null skips them; the three cand_* together)
 *    cand_R [pairs,2,3,3], cand_t, cand_n [pairs,2,3] float64 and front [cap] uint8.
 *    cap == 0 is a valid call that defines every per-pair output (the match pointers and inlier must still be non-null).  Refused
 *    before any launch (pats_last_error names the argument), in the wording and order of the pose stage: a null matches_l / matches_r /
 *    inlier / best_count / E / R / t / n / baseline / vis / sup / choice / status / front_count; matches_l / matches_r off 8 bytes, the
 *    float64 and int64 arrays, pair_off and counts_in off 8, models / best / norm / thr / vis / sup / choice / status off 4; some but not
 *    all of cand_R, cand_t, cand_n; both segment forms or neither; pairs < 1; cap < 0 or cap >= 2^31 - 1; in the strided form stride < 1 or
 *    pairs * stride > cap; swapped not 0 or 1; neither moments nor (models and best); with models given H < 1 or H > max_h; a NaN or
 *    negative min_baseline; a workspace smaller than pats_homography_pose_workspace_bytes (0 today; workspace may then be null).
 *
 * 2. pats_pose_select_by_pair: one launch, one workgroup per pair.  Inputs: the segments (as above); R_e [pairs,3,3], t_e [pairs,3],
 *    E_e [pairs,3,3] float64, front_count_e [pairs] int64, front_e [cap] uint8 (optional) of the epipolar pose with the
 *    verification's best_count_e [pairs] int64 and inlier_e [cap] uint8; the same of the planar pose (_h) with its status_h [pairs]
 *    int32; ratio [pairs] float32.
 *      epi_ok    = best_count_e >= 8
 *      planar_ok = status_h != 0
 *      branch    = planar_ok and (not epi_ok or double(best_count_h) >= double(ratio[p]) * double(best_count_e))
 *                    ? (status_h == 2 ? 3 : 2)  :  (epi_ok ? 1 : 0)
 *    - 0 no pose, 1 epipolar, 2 planar, 3 planar without a baseline (rotation only).  A NaN ratio chooses the epipolar branch when it
 *    is ok.  Outputs, every byte defined by every call: R, t, E, front_count of the chosen branch, copied as they are (branch 0: the
 *    identity, zeros and 0); branch [pairs] int32; inlier_sel [cap] uint8 and front_sel [cap] uint8 (optional; needs front_e and
 *    front_h): the chosen branch's bytes over the pair's segment, 0 everywhere else.
 *    cap == 0 is a valid call.  Refused before any launch: a null required pointer, a misaligned one, front_sel without both fronts,
 *    both segment forms or neither, pairs < 1, cap out of range, a bad stride, a workspace smaller than
 *    pats_pose_select_workspace_bytes (0 today). */
size_t pats_homography_pose_workspace_bytes(int64_t pairs, int64_t cap);
int pats_homography_pose_by_pair_f64(const float* matches_l, const float* matches_r, const uint8_t* inlier, const int64_t* pair_off,
                                     int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const int64_t* best_count,
                                     const double* moments, const float* models, int64_t H, const int32_t* best, const float* norm,
                                     const float* thr, int swapped, double min_baseline, double* E, double* R, double* t, double* n,
                                     double* baseline, int32_t* vis, int32_t* sup, int32_t* choice, int32_t* status,
                                     int64_t* front_count, double* cand_R, double* cand_t, double* cand_n, uint8_t* front,
                                     void* workspace, size_t workspace_bytes, pats_stream_t stream);
size_t pats_pose_select_workspace_bytes(int64_t pairs, int64_t cap);
int pats_pose_select_by_pair(const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap,
                             const double* R_e, const double* t_e, const double* E_e, const int64_t* front_count_e,
                             const uint8_t* front_e, const int64_t* best_count_e, const uint8_t* inlier_e, const double* R_h,
                             const double* t_h, const double* E_h, const int64_t* front_count_h, const uint8_t* front_h,
                             const int32_t* status_h, const int64_t* best_count_h, const uint8_t* inlier_h, const float* ratio,
                             double* R, double* t, double* E, int64_t* front_count, int32_t* branch, uint8_t* inlier_sel,
                             uint8_t* front_sel, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair adaptive verification (ABI 8, symbols added): the two verifications above with plain RANSAC's stopping rule - a pair's
 * models are tested in rounds of round_models, and the pair stops as soon as the probability of having missed an all-inlier sample
 * falls below 1 - confidence.  On the device, on the caller's stream, no host read and no synchronisation: after two fills,
 * 2 ceil(H / round_models) launches and the mask launch (rounds after every pair has stopped still launch; their workgroups
 * return at once).  The hypotheses are still all generated up front; only their verification stops early.
 * pats_epipolar_score_adaptive_by_pair_f32 and pats_homography_score_adaptive_by_pair_f32 take the arguments of
 * pats_epipolar_score_by_pair_f32 / pats_homography_score_by_pair_f32 in their order and meaning - the segment, norm, min_conf, thr
 * and the models models[p, 0..H-1] are exactly what those take - and then
 *   confidence         double, strictly between 0 and 1
 *   sample_size s      1 .. 16: the matches one sample draws (8, 5 or 4 for the three samplers)
 *   models_per_sample g  1 .. 16: the models one sample yields (10 for the 5-point models, otherwise 1)
 *   round_models B     a positive multiple of 64; ceil(H / B) is at most 256
 *   used, participating [pairs] int32 outputs, required
 * The rule.  All its arithmetic is IEEE float64, no contraction, no transcendental function: a host reproduces it bit for bit.
 *   participating[p]  int32: matches of the segment that take part (the verification's finite / min_conf rule). 0 when thr[p] is NaN or negative
 *   round r           tests models [r B, min(H, (r+1) B)) of every pair that has not stopped.  T_r = min(H, (r+1) B)
 *   after round r     c = the largest count over models [0, T_r), lowest index among equals (running best: a later equal count never replaces it)
 *                     k = T_r / g (integer division);  eta = 1.0 - confidence
 *                     w = (double)c / (double)participating[p]   (0 when participating is 0)
 *                     ws = w multiplied by itself s - 1 times, left to right;  q = 1.0 - ws
 *                     miss = q^k by square-and-multiply from k's most significant bit (start 1.0; per bit: square, then multiply by q if the bit is set); k = 0 gives 1.0
 *                     the pair stops iff miss <= eta
 *   used[p]           int32: T_r of the round after which the pair stopped; H if it never did
 *   counts[p, h]      as the existing verification for h < used[p]; exactly 0 for h >= used[p]
 *   best, best_count, inlier, moments
 *                     bit for bit what the existing verification returns for the same call with models[p, used[p]:] replaced by zero models
 * A pair with no inliers has q = 1 and never stops: used = H.  It still costs next to nothing - the score workgroups return on a
 * bad thr and on empty tiles.  The criterion is plain RANSAC's, also on progressive samples (it is not PROSAC's).
 * cap == 0 is a valid call and defines every per-pair output: used = H, participating = 0.
 * Refused before any launch (pats_last_error names the argument): everything the fixed-budget entries refuse (the grid is
 * ceil(longest / 2048) * pairs * ceil(min(B, H) / 256) workgroups per round); a confidence not strictly between 0 and 1 (NaN included);
 * sample_size or models_per_sample outside 1 .. 16; a round_models that is not a positive multiple of 64; more than 256 rounds; a null
 * used / participating or one off 4 bytes; a workspace smaller than pats_*_score_adaptive_workspace_bytes (one int32 per pair: the
 * stopped flags; the running best lives in best / best_count), null or off 4 bytes. */
size_t pats_epipolar_score_adaptive_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_epipolar_score_adaptive_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                             int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                             int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                             int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                             void* workspace, size_t workspace_bytes, pats_stream_t stream, double confidence,
                                             int sample_size, int models_per_sample, int64_t round_models, int32_t* used,
                                             int32_t* participating);
size_t pats_homography_score_adaptive_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_homography_score_adaptive_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                               int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                               int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                               int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                               void* workspace, size_t workspace_bytes, pats_stream_t stream, double confidence,
                                               int sample_size, int models_per_sample, int64_t round_models, int32_t* used,
                                               int32_t* participating);

/* ------------------------------------------------------------------------------------------
 * Per-pair MSAC scoring (ABI 8, symbols added): the two fixed-budget verifications with the winner chosen by how well its inliers
 * fit, not only by how many it has - the MSAC gain, sum over the inliers of 1 - e^2 / thr^2 (e^2 the squared Sampson error or the
 * squared forward transfer error).  Two models with the same support are told apart, and with a threshold a few times the noise a
 * slightly wrong model that collects an inlier or two more than the right one no longer wins.  On the device, no host read.
 * pats_epipolar_score_msac_by_pair_f32 and pats_homography_score_msac_by_pair_f32 take the arguments of
 * pats_epipolar_score_by_pair_f32 / pats_homography_score_by_pair_f32 in their order and meaning through `stream` - the matches, the
 * two segment forms and their clamping, norm, min_conf, thr, models [pairs,H,3,3], H <= pats_epipolar_max_h(), the "participates"
 * rule - and then gains and best_gain.  The verdict is the family's: inlier iff w > 0 and s <= lim, by the device function the count
 * entries run (Epipolar: s = r^2, w = den, lim = thr^2 den;  Homography: s = d0^2 + d1^2, w = a2^2, lim = thr^2 a2^2).
 * Per pair p, model h and match i
 *   a non-inlier   g_i = 0: a match that does not participate, a NaN anywhere, a zero model, a NaN or negative thr
 *   an inlier      u = s / lim for lim > 0, u = 0 for lim == 0 (thr == 0: an inlier has s == 0), in float32 and in ONE form for every
 *                  cell: u = s * rcp(lim), rcp the device's reciprocal instruction (v_rcp_f32: within 1 ulp of 1 / lim), then one
 *                  rounded multiply.  Against the exact quotient of the float32 s and lim that is a relative error of at most
 *                  3 * 2^-24.  (A lim below the smallest normal float32 may give rcp = +inf; u = 0 * inf = NaN counts as u = 1.)
 *                  q = min((uint32)floor(u * 2^20), 2^20),  g_i = 2^20 - q    (u * 2^20 is exact)
 *   gains[p, h]    int64 = sum over i of g_i.  Integer adds are order-independent: a call is bit-reproducible and a pair's gains do not
 *                  depend on where its segment lies.  pats_msac_gain_one() returns 1 << 20: gains / 2^20 ~ sum over the inliers of
 *                  1 - e^2 / thr^2, and participating - gains / 2^20 is the MSAC cost
 *   best[p]        int32: the lowest index with the largest gain; 0 when every gain is 0
 *   best_gain[p]   int64 = gains[p, best[p]];  best_count[p] int64 = counts[p, best[p]]
 *   counts [pairs,H] int32   bit for bit what the count entry returns for the same call
 *   inlier, moments          the count entries' mask kernel run on the MSAC winner: bit for bit what the count entry returns when
 *                  models[p, best[p]] is the pair's only model
 * A pair whose thr is NaN or negative has gains 0, best 0, best_gain 0, best_count 0, mask 0, moments 0.  Every call defines every
 * byte of every output, cap == 0 included (gains 0, best 0).  Like the count entries' verdicts, a gain is evaluated in float32 with
 * fused multiply-adds: docs/parity.md ("MSAC scoring") bounds its distance from a float64 evaluation per cell.
 * Refused before any launch: everything the count entries refuse, in their wording (under the MSAC entry's name) and order; then a
 * null gains / best_gain or one off 8 bytes.  Workspace: that of the count sibling (0 today; workspace may be null).
 * The adaptive entries and the local optimisation still rank by count: their stopping rule and their choice of round are defined on
 * it. */
int64_t pats_msac_gain_one(void);
int pats_epipolar_score_msac_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                         int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                         int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                         int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                         void* workspace, size_t workspace_bytes, pats_stream_t stream, int64_t* gains,
                                         int64_t* best_gain);
int pats_homography_score_msac_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                           int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models,
                                           int64_t H, const float* thr, const float* norm, int use_min_conf, float min_conf,
                                           int32_t* counts, int32_t* best, int64_t* best_count, uint8_t* inlier, double* moments,
                                           void* workspace, size_t workspace_bytes, pats_stream_t stream, int64_t* gains,
                                           int64_t* best_gain);

/* ------------------------------------------------------------------------------------------
 * Per-pair local optimisation (ABI 8, symbols added): the rounds "refit the winner's inliers, verify the refit" that follow a
 * verification - LO-RANSAC's inner loop in its simplest form - walked by ONE launch per call with the pair's matches resident on
 * chip, and the BEST round kept: the result never has less support than the model it started from.  No new numerics: every value
 * returned is one the entry points above produce, and a caller who chains them gets the same bits.  On the device, no host read.
 * What it is not: no shrinking threshold, no inner RANSAC on the inlier set, no PROSAC rule, and nothing in pipeline.forward_* or
 * the drop-in calls it.  Uncalibrated callers use pats_fundamental_polish_by_pair_f32 ("Per-pair fundamental matrices" below).
 * pats_epipolar_polish_by_pair_f32 (family F = Epipolar, min_F = 8) and pats_homography_polish_by_pair_f32 (F = Homography,
 * min_F = 4) take the verification's match, segment, thr, norm and min_conf arguments - the same two segment forms, the same
 * clamping, the same rule for a match that participates - and then
 *   models [pairs,H,3,3] float32, 1 <= H <= pats_epipolar_max_h(), and best [pairs] int32 (clamped to 0 .. H-1; null is allowed
 *              with H == 1 only): the verification's models and winner - the start of the walk.  The models are expected finite
 *   rounds     T, 1 <= T <= 16
 * Definition, per pair p
 *   support(m)   (c, M, mask): the count, the 9x9 float64 moments and the inlier bytes that pats_{epipolar,homography}_score_by_pair_f32
 *                returns for pair p when m is its one model (H = 1, moments requested) - bit for bit, the moments in that kernel's
 *                fixed order (thread-local in index order over a 512-thread walk, the xor tree over the wave, the waves in order)
 *   refit_E(M, c)  float32 cast (round to nearest even) of the E that pats_epipolar_pose_by_pair_f64 returns for (moments = M,
 *                best_count = c, swapped = 0): smallest eigenvector, nearest essential matrix, |E|_F = 1, sign rule.  "No pose"
 *                there (c < 8, non-finite, s2 == 0) gives the zero model
 *   refit_H(M, c)  float32 cast of the H that pats_homography_refit_by_pair_f64 returns for (moments = M, best_count = c,
 *                swapped = 0); "no model" there gives the zero model
 *   m_0          models[p, clamp(best[p], 0, H-1)]                      (c_0, M_0, mask_0) = support(m_0)
 *   round r = 1 .. T:   m_r = refit_F(M_{r-1}, c_{r-1});   (c_r, M_r, mask_r) = support(m_r)
 *                a zero m_r has support 0, so every later round is zero as well: the walk ends there
 *   b            the lowest r in 0 .. T with the largest c_r       (round 0 is the input: the result never has less support than it)
 * A NaN or negative thr[p] gives c_r = 0 for all r, b = 0 and model = m_0.  When m_r equals m_{r-1} bit for bit every later round
 * repeats it; the kernel stops there and copies the count into the rest of counts[p, :] - the definition cannot tell the difference.
 * There is no other early exit.  No output ever holds a NaN or an infinity.
 * Outputs - every call defines every byte of every output
 *   model [pairs,3,3] float32      m_b: a model for the verification, the pose and the refit as it stands
 *   best_count [pairs] int64       c_b
 *   inlier [cap] uint8             mask_b; 0 outside every segment and in the slack of strided rows.  Its sum over a segment is c_b
 *   moments [pairs,9,9] float64    M_b: with best_count the input of pats_epipolar_pose_by_pair_f64 / pats_homography_refit_by_pair_f64
 *   best_round [pairs] int32       b
 *   counts [pairs, T+1] int32      c_0 .. c_T
 * cap == 0 is a valid call that defines every per-pair output (the match pointers and inlier must still be non-null).  Refused
 * before any launch (pats_last_error names the argument), in the verification's wording and order: a null matches_l / matches_r /
 * models / thr / model / best_count / inlier / moments / best_round / counts; matches_l / matches_r off 8 bytes (read as float2),
 * models / thr / model / best_round / counts / conf / norm / best off 4, best_count / moments / pair_off / counts_in off 8; both
 * segment forms or neither; pairs < 1; cap < 0 or cap >= 2^31 - 1; in the strided form stride < 1 or pairs * stride > cap; H < 1 or
 * H > max_h; use_min_conf without conf; a negative or NaN min_conf; rounds outside 1 .. 16; a null best with H > 1.  The workspace is
 * pats_*_polish_workspace_bytes (0 today: a pair's walk lives in its workgroup's LDS and registers; workspace may be null).
 * PATS_ERR_UNSUPPORTED if the device does not grant a workgroup 131072 bytes of dynamic LDS (the staging of 8192 matches; a longer
 * segment is legal and is walked in global memory instead, with the same results). */
size_t pats_epipolar_polish_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_epipolar_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                     int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                     const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                     const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                     double* moments, int32_t* best_round, int32_t* counts, void* workspace, size_t workspace_bytes,
                                     pats_stream_t stream);
size_t pats_homography_polish_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_homography_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                       int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                       const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                       const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                       double* moments, int32_t* best_round, int32_t* counts, void* workspace, size_t workspace_bytes,
                                       pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair 7-point hypotheses (ABI 8, symbols added): the uncalibrated sibling of the per-pair hypotheses - for every pair p and every
 * sample h in 0 .. H-1 SEVEN distinct matches of the pair are drawn and the real fundamental matrices through them, at most three,
 * are written as row-major 3x3 models: rank 2 by construction, the cheapest epipolar sample RANSAC can use.  What
 * cv2.findFundamentalMat's RANSAC solves per sample.  One launch, no host read, no workspace, deterministic.  No calibration is
 * needed: norm is the verification's normalisation, whatever it is (advice for uncalibrated callers: INTEGRATION.md).
 * What it is not: epipoles, rectification, self-calibration (the plane-and-parallax check is a stage of its own: "Per-pair
 * plane-and-parallax hypotheses and hand-over" below).
 *   x          the verification's point, formed exactly as there: ((p0 - c0) * s0, (p1 - c1) * s1, 1) in float32 - one subtract,
 *              then one multiply, never contracted - or (p0, p1, 1) without norm.  The segment of pair p (n rows from lo on) in the
 *              same two forms, ragged (pair_off) or strided (stride, counts_in), with the same clamping as above
 *   pool       m_h = n (progressive == 0)  or  max(7, (n (h + 1) + H - 1) / H)  in int64 arithmetic
 *   sampler    the hypotheses' with seven draws: k = mix(mix(mix(s_lo) ^ s_hi) + h),  u_t = mix(k + 0x9e3779b9 (t + 1)),
 *              j_t = (uint64(u_t) (m_h - t)) >> 32,  t = 0 .. 6,  draw t = the j_t-th index of 0 .. m_h - 1 not drawn before: the
 *              first seven draws of the 8-point sample with the same seed, h and pool
 *   sample_idx [pairs,H,7] int32 (optional: null skips it), the draws in draw order;  -1 for n < 7
 *   A7         [7,9] float64, row t = vec(x_r x_l^T) of draw t (q[3i + j] = x_r[i] x_l[j]; exact products of the float32 points)
 *   basis      F1, F2: an orthonormal basis of the null space of A7 (the last two columns of Q of a Householder QR of A7^T: two
 *              orthonormal vectors orthogonal to every row whatever the rank)
 *   solutions  every real (a : b) with det(a F1 + b F2) = 0 - a binary cubic, one or three real roots; a vanishing leading
 *              coefficient is a root at infinity of b / a and the root 0 of a / b, never a division by zero.  F = a F1 + b F2
 *              scaled to |F|_F = 1, the component of largest magnitude positive (the lowest index among equals, judged on the
 *              float32 values written); at most 3
 *   models     [pairs,H,3,3,3] float32, row-major (= [pairs, 3 H, 3, 3]: a `models` argument of pats_epipolar_score_by_pair_f32 as
 *              it stands).  The solutions found occupy the lowest slots of their sample, every other slot is nine exact zeros.
 *              Order: first the roots with |b / a| <= 1 by ascending b / a, then those with |a / b| <= 1 by ascending a / b.  A
 *              solution within 1 - |<a, b>| <= 2e-6 of one already stored for its sample is not stored again (a double root; a
 *              root with |a| = |b|, which both ranges hold)
 *   n_models   [pairs,H] int32 (optional: null skips it): the number of non-zero slots
 *   zero       all three slots zero (n_models 0): n < 7 (sample_idx -1);  a sample with a non-finite coordinate after norm
 *              (sample_idx still written);  a cubic that vanishes identically or has a non-finite coefficient.  A rank-deficient
 *              sample (seven copies of one match) gives zeros or finite unit models.  Never a NaN or an infinity
 *   contract   every non-zero model e, promoted to float64, with A7 formed exactly from the float32 points:
 *                | |e| - 1 | <= 1e-5
 *                |A7 e|_2    <= B_epi eps32 |A7|_F
 *                |det F|     <= B_det eps32
 *              The solve is float64 throughout (null space by Householder QR, the cubic's coefficients from the cofactors, its
 *              critical points from one square root, a bracketed Newton iteration of at most 64 steps per monotone piece: no
 *              closed form with acos or cbrt).  Rounding a rank-2 unit matrix to float32 moves its determinant by at most
 *              eps32 / 4.  Completeness is a tested share (docs/parity.md), not a pointwise promise.  The tests hold B_epi and
 *              B_det to 8 times what a float64 LAPACK solve, rounded to float32, reaches on the same samples
 *   limits     1 <= H and 3 H <= pats_epipolar_max_h()
 * Adaptive verification of these models needs nothing new: pats_epipolar_score_adaptive_by_pair_f32 with sample_size = 7,
 * models_per_sample = 3 and round_models a multiple of 64 - 192 keeps the rounds on sample boundaries.
 * Outputs - every call defines every byte of all three.  cap == 0 is a valid call (every model zero; the match pointers must still
 * be non-null).  Refused before any launch (pats_last_error names the argument), in the wording and order of
 * pats_epipolar_hypotheses5_by_pair_f32: what that refuses, with 3 H > max_h in place of 10 H > max_h; a workspace smaller than
 * pats_epipolar_hypotheses7_workspace_bytes (0 today: a sample lives in its thread's registers; workspace may then be null).  The
 * kernel uses no LDS: there is no PATS_ERR_UNSUPPORTED case. */
size_t pats_epipolar_hypotheses7_workspace_bytes(int64_t pairs, int64_t H);
int pats_epipolar_hypotheses7_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                          const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                          const float* norm, int progressive, float* models, int32_t* sample_idx, int32_t* n_models,
                                          void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair fundamental matrices (ABI 8, symbols added): the result of the epipolar stages for a caller without intrinsics - the
 * least-squares refit of the winner's moments truncated to rank 2, taken back to the stored coordinates the way the homography
 * refit does, and the local optimisation that refits with it.  The sibling of pats_homography_refit_by_pair_f64: the same launch
 * shape (one wave per pair), the same Jacobi, the same arguments with two outputs more.  On the device, float64, no host read.
 * What it is not: epipoles, rectification, self-calibration from F.
 * pats_fundamental_refit_by_pair_f64 - best_count [pairs] int64 and moments [pairs,9,9] float64 (or, moments null, models
 * [pairs,H,3,3] float32 with best [pairs] int32) as pats_epipolar_score_by_pair_f32 or a local optimisation returned them; norm
 * [pairs,8] float32 or null, what the verification was given; swapped 0 or 1.  Per pair p
 *   f_refit   [pairs,9] float64 (optional output: null skips it): the unit eigenvector of moments[p] for its smallest eigenvalue,
 *             the lowest index among equals (only the upper triangle of moments[p] is read); without moments
 *             models[p, clamp(best[p], 0, H-1)] promoted, as it stands
 *   sigma     [pairs,3] float64: the singular values of f_refit as a row-major 3x3, descending
 *   F         [pairs,3,3] float64 = U diag(s1, s2, 0) V^T of f_refit, rescaled to |F|_F = 1, the component of largest magnitude
 *             positive (the lowest index among equals: the homography refit's sign rule).  Cast to float32 it is a model for
 *             pats_epipolar_score_by_pair_f32
 *   F_px      [pairs,3,3] float64 (optional output: null skips it) = N_r^T F N_l rescaled to Frobenius norm 1, the same sign rule,
 *             N = [[s0, 0, -c0 s0], [0, s1, -c1 s1], [0, 0, 1]] per side from norm[p] (float32 widened exactly): the fundamental
 *             matrix of the stored (c0, c1) coordinates, x_r^T F_px x_l = 0 on them.  F itself without norm
 *   eig       [pairs,2] float64: the two smallest eigenvalues of moments[p], ascending (0, 0 without moments)
 *   no model  best_count[p] < 8, a non-finite moment (upper triangle) or a non-finite f_refit, s2 == 0 (rank below 2; the zero
 *             model): zeros in F, F_px, eig, sigma and f_refit.  F_px alone is zero as well when the denormalisation is not
 *             finite or a scale of norm[p] is zero (N is then singular: no change of coordinates).  Never a NaN or an infinity
 *   swapped   1: the points were in (y, x) order - F and F_px are returned as P F P, P = [[0,1,0],[1,0,0],[0,0,1]], with the sign
 *             rule applied after the permutation; sigma, eig and f_refit do not change
 * Accuracy, as the tests hold it: | |F| - 1 | and |det F| <= 64 eps64; F within 64 eps64 / (sigma2 - sigma3) (Wedin) of LAPACK's
 * truncated SVD of the same f_refit; sigma within 64 eps64; eig and the eigen-residual of f_refit as for the homography refit.
 * Refused before any launch, in the wording and order of pats_homography_refit_by_pair_f64: a null best_count / F / eig / sigma;
 * best_count / moments / F / F_px / eig / sigma / f_refit off 8 bytes, models / best / norm off 4; pairs < 1; swapped not 0 or 1;
 * neither moments nor (models and best); with models H < 1 or H > max_h; a workspace smaller than
 * pats_fundamental_refit_workspace_bytes (0 today; workspace may be null).
 * pats_fundamental_polish_by_pair_f32 - "Per-pair local optimisation" above with family F = Fundamental, min_F = 8: the Epipolar
 * family's support (the same Sampson test, the same moments) and
 *   refit_F(M, c)  float32 cast (round to nearest even) of the F that pats_fundamental_refit_by_pair_f64 returns for (moments = M,
 *                best_count = c, swapped = 0); "no model" there gives the zero model
 * Arguments, outputs, refusals and wording are those of pats_epipolar_polish_by_pair_f32; moments and best_count are the input of
 * pats_fundamental_refit_by_pair_f64.  A caller who chains pats_epipolar_score_by_pair_f32 (H = 1, moments) and
 * pats_fundamental_refit_by_pair_f64 round for round gets the same bits. */
size_t pats_fundamental_refit_workspace_bytes(int64_t pairs);
int pats_fundamental_refit_by_pair_f64(const int64_t* best_count, const double* moments, const float* models, int64_t H,
                                       const int32_t* best, const float* norm, int64_t pairs, int swapped, double* F, double* F_px,
                                       double* eig, double* sigma, double* f_refit, void* workspace, size_t workspace_bytes,
                                       pats_stream_t stream);
size_t pats_fundamental_polish_workspace_bytes(int64_t pairs, int64_t H, int64_t cap);
int pats_fundamental_polish_by_pair_f32(const float* matches_l, const float* matches_r, const float* conf, const int64_t* pair_off,
                                        int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* thr,
                                        const float* norm, int use_min_conf, float min_conf, const float* models, int64_t H,
                                        const int32_t* best, int rounds, float* model, int64_t* best_count, uint8_t* inlier,
                                        double* moments, int32_t* best_round, int32_t* counts, void* workspace, size_t workspace_bytes,
                                        pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair plane-and-parallax hypotheses and hand-over (ABI 8, symbols added): the uncalibrated branch's answer to a dominant plane
 * (DEGENSAC: Chum, Werner, Matas, CVPR 2005).  Five or more of a 7-point sample on one plane give a family of fundamental matrices;
 * verification crowns one that explains the plane and a few accidental points.  The plane's homography and TWO matches off the plane
 * fix the epipolar geometry instead.  Two entries, each one workgroup per pair and one launch for the batch, no host read, no
 * workspace, deterministic.
 * What it is not: a sample-level H-degeneracy test of the seven points; a gate (the stage always runs, support alone decides); a
 * calibrated variant (the calibrated branch has pats_pose_select_by_pair).
 * pats_plane_parallax_hypotheses_by_pair_f32 - the arguments of pats_epipolar_hypotheses7_by_pair_f32 without progressive and
 * n_models, and the plane: models_h [pairs,Mh,3,3] float32 with best_h [pairs] int32 as pats_homography_score_by_pair_f32 or the
 * homography's local optimisation left them, thr [pairs] float32, and the host scalar parallax >= 1 (2 is the usual choice).  Per pair p
 *   x, segment  as in "Per-pair 7-point hypotheses"
 *   plane       Hp = models_h[p, clamp(best_h[p], 0, Mh-1)]; nine exact zeros are "no plane"
 *   pool        match i of the segment is a member iff its four coordinates are finite after norm and it is off the plane at
 *               parallax thr[p]:  d0^2 + d1^2 > t2 a2^2  or  a2^2 == 0,  with a = Hp x_l, d = (a0 - x_r0 a2, a1 - x_r1 a2),
 *               t2 = (parallax thr[p])^2 - every operation the float32 FMA expression of the homography verification
 *               (pats_homography_score_by_pair_f32), the products parallax thr[p] and its square rounded to float32.  A NaN on
 *               either side of the comparison is no member.  The members in ascending i are the pool; its size is written to
 *   pool_out    `pool` [pairs] int32, BEFORE clamping.  Only the first pats_plane_parallax_pool_max() (8192) members are drawn from:
 *               m = min(pool size, pool_max)
 *   sampler     the hypotheses' with two draws on 0 .. m - 1 (k, u_t, j_t as in "Per-pair 7-point hypotheses", t = 0, 1): draw t is
 *               the j_t-th member of the pool not drawn before
 *   sample_idx  [pairs,H,2] int32 (optional: null skips it): the two draws as positions inside the pair's SEGMENT, in draw order;
 *               -1, -1 when m < 2 or there is no plane
 *   solve       in float64 from the float32 points and Hp widened exactly:  a_i = Hp x_i,  l_i = x'_i x a_i  (the line through a match
 *               and its transfer: it holds the epipole),  e = l_1 x l_2,  F = [e]x Hp (column j of F = e x column j of Hp)
 *   models      [pairs,H,3,3] float32: F scaled to |F|_F = 1, the component of largest magnitude positive (the lowest index among
 *               equals, judged on the float32 values written) - a `models` argument of pats_epipolar_score_by_pair_f32
 *   zero        nine exact zeros: m < 2; no plane; |e| <= 1e-9 |l_1| |l_2| (the two parallax lines coincide); a non-finite value.
 *               Never a NaN or an infinity
 *   limits      1 <= H <= pats_epipolar_max_h(), 1 <= Mh <= pats_epipolar_max_h()
 * Outputs - every call defines every byte of models, pool and (if given) sample_idx.  cap == 0 is a valid call.  Refused before any
 * launch (pats_last_error names the argument): what pats_epipolar_hypotheses7_by_pair_f32 refuses, in its order and wording (with H
 * itself against max_h); then parallax not finite or below 1; Mh outside 1 .. max_h; a null or misaligned (4 bytes) models_h, best_h
 * or thr; a null or misaligned pool.  The kernel's LDS is static (32 KiB for the list): there is no PATS_ERR_UNSUPPORTED case.
 * pats_plane_parallax_select_by_pair - the hand-over.  a = the standing verification of the pair's fundamental matrices, b = the
 * verification of the plane-and-parallax models, each as pats_epipolar_score_by_pair_f32 left it: models_x [pairs,Hx,3,3] with
 * best_x [pairs] int32, best_count_x [pairs] int64, inlier_x [cap] uint8 and (optional) moments_x [pairs,9,9] float64.  Per pair p
 *   replaced    [pairs] uint8 = 1 iff best_count_b[p] > best_count_a[p] - strictly: a tie keeps the standing verification
 *   kept        b where replaced, else a
 *   best_count  [pairs] int64, inlier [cap] uint8 (the kept mask on the pair's segment as 0 / 1, 0 on every row outside the segments),
 *               moments [pairs,9,9] float64 (optional: null skips it; needs moments_a and moments_b), model [pairs,3,3] float32 =
 *               models_kept[p, clamp(best_kept[p], 0, H_kept - 1)]: the verification's standard form with H = 1 and best = 0
 *   overlap     [pairs] int32: the matches of the segment with inlier_a != 0 and finite coordinates that are inliers of the plane at
 *               thr[p] by the homography verification's test (a2^2 > 0 and d0^2 + d1^2 <= thr^2 a2^2; none for a NaN or negative
 *               thr or without a plane) - the standing model's degeneracy measure, to be divided by best_count_a
 * Every output byte of every pair is written; cap == 0 and zero counts are valid.  Refused before any launch: a null or misaligned
 * required pointer in the order matches_l, matches_r, models_a, best_a, best_count_a, inlier_a, models_b, best_b, best_count_b,
 * inlier_b, model, best_count, inlier, replaced, overlap; a misaligned norm, pair_off, counts_in, moments_a, moments_b, moments; the
 * segments as everywhere; Ha, Hb outside 1 .. max_h; moments without moments_a and moments_b; then the plane's arguments as above. */
int64_t pats_plane_parallax_pool_max(void);
size_t pats_plane_parallax_hypotheses_workspace_bytes(int64_t pairs, int64_t H);
int pats_plane_parallax_hypotheses_by_pair_f32(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                               const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                               const float* norm, const float* models_h, int64_t Mh, const int32_t* best_h,
                                               const float* thr, float parallax, float* models, int32_t* sample_idx, int32_t* pool,
                                               void* workspace, size_t workspace_bytes, pats_stream_t stream);
int pats_plane_parallax_select_by_pair(const float* matches_l, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                       const int64_t* counts_in, int64_t pairs, int64_t cap, const float* norm, const float* models_h,
                                       int64_t Mh, const int32_t* best_h, const float* thr, const float* models_a, int64_t Ha,
                                       const int32_t* best_a, const int64_t* best_count_a, const uint8_t* inlier_a,
                                       const double* moments_a, const float* models_b, int64_t Hb, const int32_t* best_b,
                                       const int64_t* best_count_b, const uint8_t* inlier_b, const double* moments_b, float* model,
                                       int64_t* best_count, uint8_t* inlier, double* moments, uint8_t* replaced, int32_t* overlap,
                                       pats_stream_t stream);

/* attention(query, key, value) of the GNN layers (reference models/modules.py:84-88; the core of
 * MultiHeadedAttention.forward :100-105): scores = q^T k / dim**.5 per (batch, head), softmax over the
 * keys, out = prob v.  query [batch,dim,heads,n], key / value [batch,dim,heads,m] (the view
 * modules.py:101-102 makes of the projections) -> out [batch,dim,heads,n]; prob [batch,heads,n,m] is
 * written only if non-null (the reference returns it, its caller discards it).  fp32 throughout; the
 * score matrix stays in LDS (32 query rows per workgroup up to m = 1024, 16 / 8 / 4 rows beyond; m <= 8416, PATS_ERR_UNSUPPORTED
 * past that). */
int pats_attention_f32(const float* query, const float* key, const float* value, int64_t batch, int dim,
                       int heads, int n, int m, float* out, float* prob, pats_stream_t stream);

/* ---- AttentionalPropagation of the GNN layers (reference models/modules.py:91-117; section 8f rank 4) ----------
 *   message = merge(attention(proj_q(x), proj_k(source), proj_v(source)))            MultiHeadedAttention.forward :100-105
 *   delta   = mlp(cat([x, message], dim=1)),  mlp = Conv1d(2C,2C) BatchNorm1d ReLU Conv1d(2C,C)   :107-117 (MLP :57-69)
 *   out     = residual + delta  if residual != NULL  (AttentionalGNN.forward: desc = desc + delta, :131-133)
 * x [batch,C,n], source [batch,C,m] (channel-major, as the reference's Conv1d sees them), out [batch,C,n].
 * Weights are DEVICE pointers; the Conv1d matrices are handed over TRANSPOSED ([C_in][C_out], row = input channel),
 * i.e. conv.weight[:, :, 0].t().contiguous().  BatchNorm: bn_train == 0 -> bn_a / bn_b are the folded running
 * statistics (scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale); bn_train != 0 -> bn_a /
 * bn_b are gamma / beta and the batch statistics over (batch, n) are computed here with bn_eps (PATS.eval leaves the
 * third layer in train mode, models/pats.py:112-120).  The 1x1 convolutions use the contraction of pats_cost_f32 (the
 * cat is never materialised), the
 * attention core is pats_attention_f32.  C % heads == 0, C % 8 == 0, m <= 8416. */
typedef struct pats_propagation_weights {
    const float *wq_t, *bq;   /* attn.proj[0]: [C][C] transposed, [C] */
    const float *wk_t, *bk;   /* attn.proj[1] */
    const float *wv_t, *bv;   /* attn.proj[2] */
    const float *wm_t, *bm;   /* attn.merge */
    const float *w1_t, *b1;   /* mlp[0]: [2C][2C] transposed, [2C] */
    const float *bn_a, *bn_b; /* mlp[1]: [2C] each, see above */
    const float *w2_t, *b2;   /* mlp[3]: [2C][C] transposed, [C] */
} pats_propagation_weights;
size_t pats_attentional_propagation_workspace_bytes(int64_t batch, int C, int n, int m);
int pats_attentional_propagation_f32(const float* x, const float* source, int64_t batch, int C, int heads,
                                     int n, int m, const pats_propagation_weights* weights, int bn_train,
                                     float bn_eps, const float* residual, float* out, void* workspace,
                                     size_t workspace_bytes, pats_stream_t stream);

/* The same layer with the weights additionally PACKED for the matrix pipe (ABI 5): pats_propagation_pack_f32 splits every
 * Conv1d matrix into fp16 hi + lo halves in MFMA fragment order once per layer into a caller-owned, 16-byte aligned device
 * buffer of pats_propagation_packed_bytes(C, heads) bytes (C % 8 == 0, C % heads == 0; 0 = no packed form for this shape).
 * With it
 *  - at the third level's shape (C = 128, 4 heads, n = m = 65) the layer runs as ONE kernel that keeps a problem's activations in
 *    LDS from the descriptors to the output (csrc/gnn_fused.hip; q / k / v rows and the merge's columns permuted to head-major;
 *    bn_train != 0: one kernel up to the hidden tensor, then the batch-statistics passes and the last convolution);
 *  - at every other shape the six convolutions stream the packed weights from L2 straight into the matrix pipe
 *    (csrc/conv_pk.hip: 64 columns x up to 288 input channels staged whole in LDS per workgroup) and, between 97 and 160 tokens
 *    with 33 .. 80 channels per head (the fine level: [264, 145], 4 heads), the attention core keeps its scores in registers
 *    from the first product to the second (csrc/attention145.hip).
 * The packing also FOLDS the merge Conv1d into mlp[0] (modules.py:104,116: message = Wm att + bm has one consumer, hidden = W1
 * (x | message) + b1 = W1x x + (W1m Wm) att + (W1m bm + b1)): W1m Wm and the bias are formed once, in double, and kept - as fp32
 * [2C][2C] + [2C] - at the end of the packed buffer; the packed layer runs five products instead of six and differs from the
 * two-product form by fp32 rounding only (PATS_GNN_FOLD=0, read at pack time and at run time, keeps the merge as its own product).
 * The weights must not change between the packing and the calls that use it.
 * PATS_GNN_FUSED=0 / PATS_CONV_PK=0 / PATS_ATTN145=0 and launches in which an activation left the fp16 range of the split
 * operands take the composition above (same workspace; device-side flags, no host read). */
/* The layers' overflow protocol, no reference counterpart.  Mode 0 (default, "inline"): every packed call queues its fp32
 * composition behind the fast kernels, gated on a device-side flag - right without a host read, ~16 launches per layer that
 * normally do nothing.  Mode 1 ("deferred"): none is queued; a fast kernel that meets an activation beyond the fp16 range raises
 * ONE sticky flag per device, and the outputs of that call are then NOT valid.  The caller reads the flag where it synchronises
 * anyway - pats_gnn_overflows(&raised, reset): drains the device, raised = 0 / 1 - and repeats the work in mode 0 if it is up.
 * pats_set_gnn_redo_mode returns the previous mode (and leaves it unchanged for any other argument).  Process-wide. */
int pats_set_gnn_redo_mode(int mode);
int pats_gnn_overflows(int64_t* raised, int reset);
size_t pats_propagation_packed_bytes(int C, int heads);
int pats_propagation_pack_f32(const pats_propagation_weights* w, int C, int heads, void* packed, size_t packed_bytes,
                              pats_stream_t stream);
int pats_attentional_propagation_packed_f32(const float* x, const float* source, int64_t batch, int C, int heads,
                                            int n, int m, const pats_propagation_weights* w, const void* packed,
                                            int bn_train, float bn_eps, const float* residual, float* out,
                                            void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* (ABI 6) At the FINE level's shape - C = 264, 4 heads, n = m = 145 (models/second_layer.py:44,89) - and bn_train == 0 the packed
 * layer is ONE kernel (csrc/gnn_fine.hip): a persistent workgroup per CU owns a problem, the descriptors arrive as pre-split
 * fragment images by LDS DMA, every product's output lives in the accumulators, q / k / v / attention / hidden stay in a
 * per-workgroup scratch block.  The BatchNorm scale / shift applied there are the ones in `w` AT PACK TIME (eval mode).
 * pats_attentional_propagation_packed_f32 converts a layer's [batch, C, n] tensors on the way in and out;
 * pats_attentional_gnn_packed_f32 is AttentionalGNN.forward (models/modules.py:127-134: `layers` propagations on both descriptor
 * sets, cross[l] != 0 = 'cross', the residual of :133 included) with the descriptors kept in the kernel's own form between the
 * layers.  weights[l] / packed[l]: the layer's weights and its pats_propagation_pack_f32 buffer.  Returns PATS_ERR_UNSUPPORTED
 * at any other shape (nothing launched) or when the kernel's LDS attribute is refused at run time (then a workspace fill and the
 * two input conversions have already been queued: harmless, the outputs are untouched) - run the layers one by one then.  A launch that meets a non-finite value raises a
 * device-side flag; the per-layer compositions queued behind, gated on it, redo the stack (no host read).  PATS_GNN_FINE=0
 * switches the kernel off (both entry points take the round-4 kernels).
 * live (may be NULL): a device-side row count - throughput mode's row total; rows >= clamp(*live - live_off, 0, batch) of both
 * descriptor sets are not processed and their output rows are written as zeros (also when the redo chain ran; it copies the live
 * rows only).
 * pats_attentional_propagation_packed_counted_f32: one packed layer over a capacity with such a count, honoured by the one-kernel
 * layers in eval mode - output rows past the count are zeros at the fine level's shape and left untouched at the third level's,
 * also when the gated composition redoes the call (it computes into the workspace and copies the live rows out); ignored at any
 * other shape.  bn_train != 0 with a count is refused (PATS_ERR_INVALID, nothing launched). */
size_t pats_attentional_gnn_packed_workspace_bytes(int64_t batch, int C, int heads, int n);
int pats_attentional_gnn_packed_f32(const float* desc0, const float* desc1, int64_t batch, const int64_t* live, int64_t live_off,
                                    int C, int heads, int n, int layers,
                                    const pats_propagation_weights* const* weights, const void* const* packed,
                                    const int* cross, float bn_eps, float* out0, float* out1, void* workspace,
                                    size_t workspace_bytes, pats_stream_t stream);
int pats_attentional_propagation_packed_counted_f32(const float* x, const float* source, int64_t batch, const int64_t* live,
                                                    int64_t live_off, int C, int heads, int n, int m,
                                                    const pats_propagation_weights* w, const void* packed, int bn_train,
                                                    float bn_eps, const float* residual, float* out, void* workspace,
                                                    size_t workspace_bytes, pats_stream_t stream);

/* ---- the descriptor heads either side of the GNN: Conv1d(kernel_size=1) and BatchNorm1d + ReLU -------------------
 * Replaces nn.Conv1d(k=1) wherever the path uses it alone - `final_proj` right before the cost build
 * (models/first_layer.py:34-36,105; models/second_layer.py:40-42,91) - and, chained, the MLP of
 * models/modules.py:57-69 that KeypointEncoder is (:70-82; first_layer.py:30-31,81; third_layer.py:96-97,139-140):
 *   y[b][o][t] = bias[o] + sum_c w[o][c] * f(x[b][c][t]),   f(v) = v                              (in_scale == NULL)
 *                                                           f(v) = max(0, v * in_scale[c] + in_shift[c])  otherwise
 *   (+ residual[b][o][t] if residual != NULL)
 * i.e. the BatchNorm1d + ReLU that follows a Conv1d inside MLP is applied while the NEXT Conv1d stages its input:
 * eval mode  -> in_scale = gamma / sqrt(running_var + eps), in_shift = beta - running_mean * in_scale (host side);
 * train mode -> pats_bn_fold_f32 below computes them from the batch statistics of the previous layer's output.
 * x [batch,K,n], y [batch,M,n] channel-major like the reference's Conv1d; w_t = conv.weight[:, :, 0].t().contiguous()
 * ([K][M], row = input channel); bias [M] or NULL.  K % 8 == 0 (pad the two keypoint coordinates with zero channels).
 * Same contraction as pats_cost_f32.  Workspace: pats_conv1x1_workspace_bytes(). */
size_t pats_conv1x1_workspace_bytes(void);
int pats_conv1x1_f32(const float* w_t, const float* bias, const float* x, int64_t batch, int K, int M, int n,
                     const float* in_scale, const float* in_shift, const float* residual, float* y, void* workspace,
                     size_t workspace_bytes, pats_stream_t stream);
/* BatchNorm1d in TRAIN mode (F.batch_norm on batch statistics: per channel over (batch, n), biased variance), folded:
 * scale[c] = gamma[c] / sqrt(var_c + eps), shift[c] = beta[c] - mean_c * scale[c].  Deterministic (fixed summation
 * order, double accumulation).  PATS.eval() leaves the third layer in train mode (models/pats.py:112-120), so its
 * KeypointEncoder normalises with these. */
size_t pats_bn_fold_workspace_bytes(int C);
int pats_bn_fold_f32(const float* h, int64_t batch, int C, int n, const float* gamma, const float* beta, float eps,
                     float* scale, float* shift, void* workspace, size_t workspace_bytes, pats_stream_t stream);

/* ---- the scale head: target descriptors -> the OT problem's column marginals `ns` -------------------------------------
 * Replaces  scale = exp(sigmoid(proj(desc1[:, :, :h*w] as [b,C,h,w])) * ln256 - ln256 / 2)  with proj = nn.Conv2d(C, 1,
 * kernel_size=3, padding=1):  models/first_layer.py:39-40,106-107 (scalex_proj, 15x20 grid);  models/second_layer.py:33-36,
 * 92-98 (scalex_proj and scaley_proj on the 12x12 grid, scale = scale_x * scale_y: heads = 2);  models/third_layer.py:88-89,
 * 151-152 (scale_proj, 8x8).  x [batch,C,ld] is the tensor the cost build takes (ld = h*w, or h*w + 1 with the dustbin
 * feature column, which the heads skip); weight [heads][C][3][3] = the Conv2d weights concatenated over heads; bias
 * [heads]; out [batch][h*w] is `ns` as log_optimal_transport / log_optimal_transport2 take it; per_head (optional, NULL to
 * skip) [batch][heads][h*w] receives the heads on their own - scale_x and scale_y, which SecondLayer.est_position takes
 * separately (second_layer.py:116-117).  h*w <= 512. */
int pats_scale_head_f32(const float* x, int64_t batch, int C, int ld, int h, int w, const float* weight,
                        const float* bias, int heads, float* out, float* per_head, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair absolute pose from depth (ABI 8, symbols added): the left (database) image comes with a depth map, a match in it is
 * LIFTED to a metric 3-D point, three lifted matches give the right (query) camera's absolute pose (P3P) and the candidates are
 * verified by reprojection.  The result is a metric (R, t) - what the two-view stages cannot give.  Three entry points; each takes
 * the per-pair segments in the two forms of pats_epipolar_score_by_pair_f32 (ragged pair_off, or stride with counts_in, exactly
 * ONE of them, with the same clamping), issues a fixed number of launches for the whole batch and reads nothing back.
 * The refit of the winner on its inliers and its local optimisation are "Per-pair absolute local optimisation" below.
 * What it is not: MSAC, adaptive stopping, a sampler that skips invalid matches; nothing in pipeline.forward_* or the drop-in calls
 * it.
 *
 * 1. The lift.  Inputs
 *   matches [cap,2] float32   ONE side's list in the hand-over's (c0, c1) = (y, x) order, un-normalised pixels of the map
 *   norm [pairs,8] float32 (optional)   its LEFT half (c0, c1, s0, s1) normalises the point: x_k = (p_k - c_k) * s_k, one subtract and
 *              one multiply in float32, as everywhere; without it x = p
 *   depth_table [pairs,4] int64   per pair (address of a float32 map, h, w, row stride in elements): map axis 0 belongs to c0, axis 1
 *              to c1, the centre of pixel (i, j) is at (c0, c1) = (i, j).  A null address, h < 1 or w < 1: every match of the pair is
 *              invalid
 *   max_depth [pairs] float32 (optional), interp (0 nearest, 1 bilinear), use_max_jump (0 or 1) with max_jump
 * Definition, per match (p0, p1), float32 throughout, every operation rounded once, no contraction
 *   nearest    i = rint(p0), j = rint(p1) (round half to even; still float32), the tap (i, j), d = depth[i, j]
 *   bilinear   i0 = floor(p0), a = p0 - i0, j0 = floor(p1), b = p1 - j0.  The taps USED are (i0, j0), (i0, j0 + 1) if b > 0,
 *              (i0 + 1, j0) if a > 0 and (i0 + 1, j0 + 1) if both: a tap whose weight is exactly zero is not read and enters the sum
 *              as 0, so p0 = h - 1 with a = 0 is inside the map.  wa = 1 - a, wb = 1 - b, w00 = wa wb, w01 = wa b, w10 = a wb,
 *              w11 = a b;  d = ((w00 d00 + w01 d01) + w10 d10) + w11 d11  - four products, then three sums left to right
 *   invalid    iff a coordinate is not finite; a used tap lies outside [0, h) x [0, w); a used tap is not finite or <= 0; in the
 *              bilinear form with use_max_jump, (max tap - min tap) > max_jump * min tap over the used taps (a depth edge; max_jump
 *              is not looked at in the nearest form); max_depth given and d > max_depth[p] (a NaN limit does not limit); or the pair
 *              has no map
 *   point      X = (x0 d, x1 d, d): each product rounded once
 * Outputs - every call defines every byte: rows of cap in no segment (and the slack of a strided row) hold exact zeros, as
 * pats_epipolar_triangulate_by_pair_f64 leaves them; an invalid match of a segment holds three NaNs and valid = 0
 *   points [cap,3] float32,  valid [cap] uint8,  lift_count [pairs] int64 = valid's sum over the segment, exactly
 * Refused before any launch: a null matches / depth_table / points / valid / lift_count; matches, depth_table, lift_count, pair_off or
 * counts_in off 8 bytes, norm, max_depth or points off 4; the segment rules of every per-pair stage (both forms or neither, pairs < 1,
 * cap < 0 or cap >= 2^31 - 1, stride < 1 or pairs * stride > cap); interp or use_max_jump not 0 or 1.  cap == 0 is a valid call. */
int pats_lift_by_pair_f32(const float* matches, const int64_t* pair_off, int64_t stride, const int64_t* counts_in, int64_t pairs,
                          int64_t cap, const float* norm, const int64_t* depth_table, const float* max_depth, int interp,
                          int use_max_jump, float max_jump, float* points, uint8_t* valid, int64_t* lift_count, pats_stream_t stream);

/* 2. P3P hypotheses: H samples per pair, one thread each, every sample solved for the up to four (R, t) with x_r ~ R X + t.
 *   points [cap,3] float32 (the lift's), matches_r [cap,2] float32 with norm's RIGHT half (optional) as the verification normalises
 *   sampler    the one of pats_epipolar_hypotheses_by_pair_f32 with three draws: the pool is n, or with progressive
 *              max(3, ceil(n (h + 1) / H)); pair_seed [pairs] int64; sample_idx [pairs,H,3] int32 (optional) gets the draws, -1 for a
 *              pair with n < 3
 *   solve      float64, Grunert's quartic in the ratio of two camera distances, its positive real roots bracketed by the roots of its
 *              derivatives, the three distances polished on the law-of-cosines equations, the pose from the two triangles' frames
 *   kept       a sample with a non-finite point (an invalid lift) or right point gives no model.  A solution is kept iff it is finite,
 *              also as float32; the camera-frame depths of its three points are positive; and its largest reprojection residual on
 *              its own three points, max_i |(Y_i0, Y_i1) / Y_i2 - x_r,i|_inf in float64, is <= 1e-8
 *   models [pairs,H,4,3,4] float32   row-major [R | t] in the frame of the points, the kept solutions first by ascending camera
 *              distance of the first sample point, exact zero models behind; n_models [pairs,H] int32 (optional) their number
 * Refused before any launch: a null points / matches_r / pair_seed / models; matches_r, pair_seed, pair_off or counts_in off 8
 * bytes, the others off 4; the segment rules; H < 1 or 4 H above pats_epipolar_max_h; progressive not 0 or 1. */
int pats_absolute_hypotheses_by_pair_f32(const float* points, const float* matches_r, const int64_t* pair_off, int64_t stride,
                                         const int64_t* counts_in, int64_t pairs, int64_t cap, int64_t H, const int64_t* pair_seed,
                                         const float* norm, int progressive, float* models, int32_t* sample_idx, int32_t* n_models,
                                         pats_stream_t stream);

/* 3. Reprojection verification: M models [pairs,M,3,4] float32 per pair (M <= pats_epipolar_max_h) against every match.
 *   takes part a match whose X and (normalised) x_r are finite and, with use_min_conf, whose conf >= min_conf (false for a NaN)
 *   test       float32 FMAs in this order:  Y_k = fma(m[k,0], X0, fma(m[k,1], X1, fma(m[k,2], X2, m[k,3])));  d_k = fma(-r_k, Y2, Y_k)
 *              for k = 0, 1;  s = fma(d0, d0, d1 * d1);  lim = (thr * thr) * (Y2 * Y2);  inlier iff the match takes part, Y2 > 0
 *              and s <= lim - no division.  thr [pairs] float32 in normalised units; a NaN or negative thr: no inliers.  An all-zero
 *              model has Y = 0: no inliers by construction
 *   counts [pairs,M] int32;  best [pairs] int32 = the lowest index among the largest counts (0 when no model has an inlier),
 *   best_count [pairs] int64;  inlier [cap] uint8 = the winner's verdicts, zero outside the segments: its sum is best_count exactly
 * Integer sums only: two calls give the same bits.
 * Refused before any launch: a null points / matches_r / models / thr / counts / best / best_count / inlier; the alignment and
 * segment rules above; M outside 1 .. pats_epipolar_max_h; use_min_conf without conf, a negative or NaN min_conf. */
int pats_absolute_score_by_pair_f32(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off,
                                    int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t M,
                                    const float* thr, const float* norm, int use_min_conf, float min_conf, int32_t* counts,
                                    int32_t* best, int64_t* best_count, uint8_t* inlier, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair absolute local optimisation (ABI 8, a symbol added): the rounds "refit the pose on the winner's inliers by Gauss-Newton on
 * the reprojection error, verify the refit" that follow pats_absolute_score_by_pair_f32, walked by ONE launch for the whole batch -
 * one workgroup per pair, the pair's matches resident in LDS, nothing read back, no workspace, no atomics - and the best round kept.
 * The inputs up to min_conf are pats_absolute_score_by_pair_f32's, with its segments, normalisation and confidence gate; best [pairs]
 * int32 is its output (null: M == 1); T = rounds (1 .. 16); G = steps (1 .. 8; the callers' default is 3).
 *
 *   support(m)   (c, mask): what pats_absolute_score_by_pair_f32 returns for pair p when m is its one model (M = 1), bit for bit -
 *                the same loads and the same float32 test, so mask's sum is c exactly
 *   sums(m, mask)  with R, t = m in float64, over the matches of mask in the FIXED order below:  Y = R X + t, each row
 *                ((m_k0 X0 + m_k1 X1) + m_k2 X2) + m_k3;  iz = 1 / Y2,  u = Y0 iz,  v = Y1 iz;  e = (u - r0, v - r1);  the Jacobian of
 *                e for a left perturbation Y -> Y + w x Y + tau, unknowns (w0, w1, w2, tau0, tau1, tau2), which is
 *                [[1/Y2, 0, -u/Y2], [0, 1/Y2, -v/Y2]] [ -[Y]x | I ] written out:
 *                    J0 = (-u v,  1 + u u,  -v,  iz,  0,  -u iz)        J1 = (-(1 + v v),  u v,  u,  0,  iz,  -v iz)
 *                A = sum J^T J (the 21 entries of the upper triangle, row by row), b = sum J^T e (6), S = sum |e|^2 (1): 28 float64
 *                sums, every product and sum rounded once, no contraction
 *   step(m, mask)  A = L L^T in index order without pivoting; "no step" if a pivot p_k = A_kk - sum_q<k L_kq^2 is not finite or not
 *                > 1e-12 A_kk;  d = -A^-1 b by the two triangular solves;  with w = d[0:3], tau = d[3:6], th = |w|:
 *                exp([w]x) = I + (sin th / th) [w]x + (2 sin^2(th / 2) / th^2) [w]x^2 (the identity for th = 0);
 *                R' = exp([w]x) R,  t' = exp([w]x) t + tau;  "no step" if an entry of (R', t') is not finite
 *   refit(m, mask, c)  "no refit" if c < 4.  Otherwise G steps in float64, the first from m widened, ALL on the same mask (plain
 *                Gauss-Newton: no damping, no line search); then R <- R + R (I - R^T R) / 2 - one Newton step towards the nearest
 *                rotation: the steps carry the float32 input's R^T R along, eps32 off the identity, and this squares that distance,
 *                so the cast leaves |R^T R - I|_max <= 4 eps32 after any number of rounds -; then the cast to float32 (round to
 *                nearest even).  A "no step" at any of the G steps, or a cast that is not finite, is "no refit".  "No refit"
 *                returns m itself
 *   m_0          models[p, clamp(best[p], 0, M - 1)];   (c_0, mask_0) = support(m_0);   S_0 = S of sums(m_0, mask_0)
 *   round r = 1 .. T   m_r = refit(m_{r-1}, mask_{r-1}, c_{r-1});   (c_r, mask_r) = support(m_r);   S_r likewise.  The first step of
 *                round r + 1 uses the very sums whose S is S_r: one pass over the matches, not two
 *                m_r equal to m_{r-1} bit for bit ends the walk: every later round would repeat it; c and S are copied into the rest
 *   b            walking r = 0 .. T, round r replaces the best so far iff c_r is larger, or equal with S_r smaller (a NaN S_r never
 *                is): the largest c_r, among those the smallest S_r, among those the lowest r.  Round 0 is the input: never less support
 *   outputs      model [pairs,3,4] float32 = m_b;  best_count [pairs] int64 = c_b;  inlier [cap] uint8 = mask_b, every byte of cap
 *                written (zeros outside the segments);  best_round [pairs] int32 = b;  counts [pairs,T+1] int32 = c_0 .. c_T;
 *                cost [pairs,T+1] float64 = S_0 .. S_T
 * A NaN or negative thr[p], or an empty segment: c_r = 0, S_r = 0, b = 0, model = m_0.  c_r = 0 gives S_r = 0 (an empty sum).
 * The fixed order of the 28 sums, as "Per-pair local optimisation" fixes its moments': thread j of 512 adds the inliers among matches
 * j, j + 512, j + 1024, ... of the segment in that order; the 64 sums of a wave are added by the xor tree (lane ^ 32, ^ 16, ^ 8, ^ 4,
 * ^ 2, ^ 1); the 8 waves' sums are added in wave order starting from 0.0.  Two calls give the same bits in all six outputs; a change of
 * the walk's width or of this order changes them and is a change of this definition.
 * Refused before any launch: what pats_absolute_score_by_pair_f32 refuses of the shared arguments (a null points / matches_r / models
 * / thr; here also a null model / best_count / inlier / best_round / counts / cost; best_count and cost off 8 bytes, best off 4; the
 * segment rules; M outside 1 .. pats_epipolar_max_h; use_min_conf without conf, a negative or NaN min_conf), then rounds outside
 * 1 .. 16, steps outside 1 .. 8, a null best with M > 1.  PATS_ERR_UNSUPPORTED if the device refuses the dynamic LDS.  cap == 0 is a
 * valid call. */
int pats_absolute_polish_by_pair_f32(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off,
                                     int64_t stride, const int64_t* counts_in, int64_t pairs, int64_t cap, const float* models, int64_t M,
                                     const float* thr, const float* norm, int use_min_conf, float min_conf, const int32_t* best, int rounds,
                                     int steps, float* model, int64_t* best_count, uint8_t* inlier, int32_t* best_round, int32_t* counts,
                                     double* cost, pats_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Per-pair match error against ground truth (ABI 8, a symbol added): whether the MATCHES are right.  A left match lifted through the
 * left depth map (pats_lift_by_pair_f32) is carried through the ground-truth relative pose into the right image, and the distance of
 * the matched right point from that projection is the match's error in pixels - the reprojection form of the check the reference's
 * Compute_depth_label (datasets/megadepth.py) and Compute_label (utils/utils.py) make, and the "matching precision" every matcher
 * reports on ScanNet and MegaDepth.  The epipolar test of a verification with the ground truth's essential matrix lets a match slide
 * along its epipolar line; this does not.  With the right image's depth map the match must also be covisible.  Per pair it counts
 * the outcomes, the matches within each threshold, the same over a sweep of confidence floors (to choose min_conf, K and cell of the
 * top-K stages) and the confusion against a mask (how many of a verification's inliers are true).  The segments come in the two
 * forms of pats_epipolar_score_by_pair_f32 (ragged pair_off, or stride with counts_in, exactly ONE of them, with the same
 * clamping).  Two fills and ONE launch for the whole batch, nothing read back, no workspace, no environment switch.
 * What it is not: the right-to-left direction (call it with the sides exchanged and the inverse ground truth); a resampler - the depth
 * maps must be given at the resolution the matches live at, as for the lift; the reference's grid labels themselves; and nothing in
 * pipeline.forward_*, the drop-in, bench.py or the smoke run calls it.
 *
 * Inputs
 *   points [cap,3] float32      pats_lift_by_pair_f32's output: X = (x0 d, x1 d, d); an invalid lift holds NaNs
 *   matches_r [cap,2] float32   the right list, (c0, c1) = (y, x) un-normalised pixels: p = (p0, p1)
 *   norm [pairs,8] float32 (optional)   only its RIGHT half (c0, c1, s0, s1) is used: it takes the projection back to pixels.  Pass
 *              what the lift was given
 *   T1 [pairs,4,4], T0 [pairs,4,4] float64 (T0 optional)   as pats_pose_error_by_pair_f64 takes them; R_gt, t_gt by exactly its formula
 *   swapped (0 or 1)            1: the ground truth is in the reference's (x, y) frame and is conjugated into the frame of the points,
 *              as the pose stages do: Rg = P R_gt P, tg = P t_gt, P exchanges the first two components (an index permutation: exact).
 *              0: Rg = R_gt, tg = t_gt
 *   depth_r_table [pairs,4] int64 (optional)   the RIGHT images' depth maps in the layout of the lift's depth_table (address of a
 *              float32 map, h, w, row stride in elements).  A null address, h < 1 or w < 1: no covisibility test for that pair
 *   occl_rel (float64, finite, > 0)   looked at only with depth_r_table
 *   size_r [pairs,2] float32 (optional)   (h, w) of the right image's real content (the canvas minus its pad)
 *   conf [cap] float32 (optional), use_min_conf with min_conf   the verification's gate.  A match TAKES PART iff p0 and p1 are finite
 *              and, with use_min_conf, conf >= min_conf (false for a NaN)
 *   thr        n_thr HOST doubles, 1 <= n_thr <= 8, each finite and > 0, strictly ascending, in pixels
 *   edges (optional)   B HOST floats, 1 <= B <= 64, finite, strictly ascending: confidence floors.  Needs conf
 *   mask [cap] uint8 (optional)   e.g. a verification's inlier mask; non-zero is "in"
 * Definition, per match of a segment that takes part (float64, no contraction, sums left to right, brackets first; the float32
 * inputs are widened exactly)
 *   Y_i = ((Rg[i][0] X0 + Rg[i][1] X1) + Rg[i][2] X2) + tg[i]            i = 0, 1, 2
 *   u_k = Y_k / Y_2;   q_k = u_k / s_k + c_k  (without norm q_k = u_k);   e_k = q_k - p_k            k = 0, 1
 *   err = sqrt(e0 e0 + e1 e1)
 *   status     the first rule that applies:
 *              0  the row is in no segment, or the match does not take part
 *              2  X is not finite (no depth)
 *              3  Y_2 <= 0 or an entry of Y is not finite (behind the right camera; also a ground truth that is not finite)
 *              4  size_r given and not (0 <= q0 <= h - 1 and 0 <= q1 <= w - 1)
 *              5  the pair has a right map and the tap i = rint(q0), j = rint(q1) (round half to even, in float64) lies outside
 *                 [0, h) x [0, w) of the map, or d1 = map[i, j] is not finite or <= 0
 *              6  the pair has a right map and abs(Y_2 - d1) > occl_rel * d1 (not covisible)
 *              1  scored
 *   An err that is not finite (an overflow of finite inputs) is scored, lies within no threshold and makes err_sum not finite.
 * Outputs - every call defines every byte; rows of cap in no segment (and the slack of a strided row) hold exact zeros
 *   err [cap] float64           NaN for a row of a segment that is not scored
 *   status [cap] uint8
 *   tally [pairs,8] int64       the segment's rows per status value; slot 7 is zero
 *   correct [pairs,n_thr] int64   the scored matches with err <= thr[k]
 *   err_sum [pairs] float64     the sum of err over the scored matches (0 for none)
 *   sweep [pairs,B,1+n_thr] int64 (with edges, and only then)   sweep[p,b,0] = the scored matches with conf >= edges[b], compared in
 *              float32; sweep[p,b,1+k] = those of them with err <= thr[k].  A NaN conf is in no bin
 *   confusion [pairs,4] int64 (with mask, and only then)   over the scored matches, good = err <= thr[0]:
 *              (mask & good, mask & !good, !mask & good, !mask & !good)
 * The fixed order of err_sum, as "Per-pair absolute local optimisation" fixes its 28 sums': thread j of 256 adds the scored matches
 * among j, j + 256, j + 512, ... of the segment in that order, starting from 0.0; the 64 sums of a wave are added by the xor tree
 * (lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1); the 4 waves' sums are added in wave order starting from 0.0.  Everything else is integer.
 * Two calls give the same bits in all seven outputs; a change of the walk's width or of this order changes err_sum and is a change
 * of this definition.
 * Refused before any launch: a null points / matches_r / T1 / thr / err / status / tally / correct / err_sum; matches_r, pair_off,
 * counts_in, T1, T0, depth_r_table, err, tally, correct, err_sum, sweep or confusion off 8 bytes, points, conf, norm or size_r off 4;
 * the segment rules of every per-pair stage (both forms or neither, pairs < 1, cap < 0 or cap >= 2^31 - 1, stride < 1 or
 * pairs * stride > cap); use_min_conf without conf, a negative or NaN min_conf; swapped not 0 or 1; with depth_r_table an occl_rel
 * that is not finite and positive; n_thr outside 1 .. 8; a threshold that is not finite and positive or does not ascend; edges
 * without sweep or sweep without edges, mask without confusion or confusion without mask; edges without conf; B outside 1 .. 64; an
 * edge that is not finite or does not ascend.  cap == 0 is a valid call. */
int pats_match_error_by_pair_f64(const float* points, const float* matches_r, const float* conf, const int64_t* pair_off, int64_t stride,
                                 const int64_t* counts_in, int64_t pairs, int64_t cap, const float* norm, const double* T1,
                                 const double* T0, int swapped, const int64_t* depth_r_table, double occl_rel, const float* size_r,
                                 int use_min_conf, float min_conf, const double* thr, int64_t n_thr, const float* edges, int64_t B,
                                 const uint8_t* mask, double* err, uint8_t* status, int64_t* tally, int64_t* correct, double* err_sum,
                                 int64_t* sweep, int64_t* confusion, pats_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PATS_AMD_H */
