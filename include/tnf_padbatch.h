/* Sampling a RealNVP ("coupling") flow of any width 2 <= D <= 63 (D != 32) with FRESH batch statistics in one call:
 * NormFlow.forward(freeze_bn=False) (density_estimator.py:364-388 of the reference, BatchNorm.forward(use_last=False),
 * bijectors.py:389-426), which has one-call chains at D = 32 and 64 only (tnf_flow_forward_batch_f32 and the pair
 * tnf_flow_forward_train_fwd_f32 / _bwd_f32).  The flow is embedded into the one of width 2H with zeros in the extra
 * slots -- the layout of tnf_padtrain.h, whose embed / gather kernels move the rows and parameter rows -- and the existing
 * chains run at width 2H.  One thing does not carry over: BatchNorm over a padded column is not the identity.  The
 * existing fold derives alpha = sqrt(var_b + eps) for every column, so a zero column would get alpha = sqrt(eps), add
 * -log sqrt(eps) to the log-det and, with eps = 0, turn into NaN.  The chains here therefore use a fold of their own:
 *
 * tnf_flow_padded_batch_fold_f32: the statistics of one BatchNorm layer and the constants that fold it (and, for an odd
 *   layer, the Affine behind it) into the next kernel's load stage, from moments = [sum (2H) | sum of squares (2H) | row
 *   count] doubles of rows in the embedded layout.  At a real slot the arithmetic of the existing fold, in its order:
 *   mean and var_b in double, alpha = sqrt(var_b + eps), (float) casts, log-det -= logf(alpha).  At a padded slot
 *   mean = 0, alpha = 1, A = 1, B = 0, no log-det term, and 1 / sqrt(0 + eps) is never evaluated.  mean_out / alpha_out
 *   are (2H,) rows; fold is (M_p, 2, 2H) = [A | B]; ldc (M_p) is overwritten when `first` is non-zero, else added to.
 *   affine_off: the offset of the Affine block [alpha (2H) | shift (2H)] inside an embedded parameter row, read when
 *   has_affine is non-zero.  One launch of M_p workgroups; plain vector loads and stores, no atomics, no allocation, no
 *   synchronisation (capturable).  NULL pointers, M_p < 1, a D without an embedded layout (TNF_EUNSUPPORTED),
 *   affine_off < 0 and pstride < affine_off + 4H (with has_affine) are refused before the launch.
 * tnf_flow_padded_batch_supported(D, S, L, U): 1 exactly when tnf_flow_padded_width(D) != 0 and the existing chains
 *   accept (2H, S, L, U), i.e. tnf_flow_train_workspace_bytes(1, 1, 32, 2H, S, L, U) >= 0; else 0.
 * tnf_padbatch_launch_count(which): calls that reached their launches, per entry; a counter space of its own
 *   (TNF_DIAG_FAMILIES is a closed set).
 *
 * The two composites.  Arguments as their D = 32 / 64 counterparts (omega, z_out, g_z, g_omega (M, N, D); params
 * (M_p, pstride), M_p = 1 or M; sum_log_det (M, N); bn_mean_out / bn_alpha_out (2S, D): what each BatchNorm layer's own
 * forward(use_last=False) would have cached), except that rows need 4-byte alignment only and that `states` and `folds`
 * are kept at the embedded width: states (2S, M, N, 2H), 16-byte aligned, folds (2S, M_p, 2, 2H).  Each embeds omega and
 * the parameter rows into the workspace, runs the existing chain at width 2H with the fold above in place of the existing
 * one, and gathers z (and g_omega, g_params) back to width D; a small gather produces the (2S, D) statistics.  The
 * gradient at padding is never read back.  Refused before any launch: NULL pointers, M < 1, M_p not in {1, M}, N < 0,
 * M * N < 2 and a pstride / gpstride shorter than tnf_flow_num_params(D, S, L, U) are TNF_EINVAL; a shape for which
 * tnf_flow_padded_batch_supported is 0 is TNF_EUNSUPPORTED; a NULL, short or not 256-byte aligned workspace is
 * TNF_EWORKSPACE.  N == 0 returns TNF_OK without a launch.
 *   tnf_flow_padded_forward_batch_f32       no autograd.  z_out must not alias omega.
 *   tnf_flow_padded_forward_train_fwd_f32   the forward of the one-node pair: keeps states and folds.
 *   tnf_flow_padded_forward_train_bwd_f32   its backward from g_z and g_sum_log_det: g_omega (optional) and g_params
 *                                           (M_p, gpstride; the real row is written over).  bn_mean / bn_alpha: the
 *                                           (2S, D) rows the forward wrote; embedded with (0, 1) at padding, so that
 *                                           P = Q = 0 and v = 0 there and the fold's backward leaves the padded
 *                                           gradient columns at exactly 0.
 *   tnf_flow_padded_batch_workspace_bytes / tnf_flow_padded_batch_train_workspace_bytes: their workspaces -- the embedded
 *   rows, parameter (and gradient) rows and statistics, and the workspace of the chain at width 2H; TNF_EINVAL /
 *   TNF_EUNSUPPORTED as above.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * PADBATCH_SIGNATURES; tests/test_padded_batch_host.py keeps this header, the exports and that table in step.
 * float32 only. */
#ifndef TNF_PADBATCH_H
#define TNF_PADBATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    TNF_PADBATCH_COUNT_FOLD = 0,
    TNF_PADBATCH_COUNT_GATHER_STATS = 1,
    TNF_PADBATCH_COUNT_FORWARD = 2,
    TNF_PADBATCH_COUNT_TRAIN_FWD = 3,
    TNF_PADBATCH_COUNT_TRAIN_BWD = 4,
    TNF_PADBATCH_COUNTERS = 5
};
int tnf_flow_padded_batch_supported(int32_t D, int32_t S, int32_t L, int32_t U);
int64_t tnf_padbatch_launch_count(int32_t which);
int tnf_flow_padded_batch_fold_f32(const float* params, const double* moments, float* mean_out, float* alpha_out,
                                   float* fold, float* ldc, int64_t M_p, int32_t D, int64_t pstride, int64_t affine_off,
                                   int32_t has_affine, int32_t first, float eps, void* stream);
int64_t tnf_flow_padded_batch_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U);
int tnf_flow_padded_forward_batch_f32(const float* omega, const float* params, float* z_out, float* sum_log_det,
                                      float* bn_mean_out, float* bn_alpha_out, int64_t M, int64_t M_p, int64_t N, int32_t D,
                                      int32_t S, int32_t L, int32_t U, int64_t pstride, float eps, void* workspace,
                                      int64_t workspace_bytes, void* stream);
int64_t tnf_flow_padded_batch_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L,
                                                    int32_t U);
int tnf_flow_padded_forward_train_fwd_f32(const float* omega, const float* params, float* z_out, float* sum_log_det,
                                          float* states, float* folds, float* bn_mean_out, float* bn_alpha_out, int64_t M,
                                          int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride,
                                          float eps, void* workspace, int64_t workspace_bytes, void* stream);
int tnf_flow_padded_forward_train_bwd_f32(const float* omega, const float* params, const float* states, const float* folds,
                                          const float* bn_mean, const float* bn_alpha, const float* g_z,
                                          const float* g_sum_log_det, float* g_omega, float* g_params, int64_t M, int64_t M_p,
                                          int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride,
                                          int64_t gpstride, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_PADBATCH_H */
