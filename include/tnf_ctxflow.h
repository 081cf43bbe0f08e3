/* Per-context RealNVP ("coupling") flows with few samples per context, one launch per call: one parameter row per
 * context m and 1 <= N <= 31 rows of z per context -- ConditionalDensityEstimator.log_prob(z (M, N, D), x),
 * cde(x, N, freeze_bn=True) and cde.sample(x, N) -- at every width 2 <= D <= 64.  The one-call kernels of tnf.h leave this
 * layout to the per-bijector composition (5 S launches): their prepared operand images, ~100 KB per context, would
 * outweigh the samples.  Here one wave serves one context: it loads the context's rows once, walks the 2 S coupling layers
 * in the call's direction with the exact-f32 MFMA tile, gathering each layer's operands straight from the context's packed
 * parameter row (real half widths h = D / 2 and D - h, zero-padded to 16 or 32), applies the BatchNorm / Affine maps
 * between layers in registers and writes its outputs once.  No prepared images, no workspace, no second launch: a
 * parameter row leaves HBM once and each z row is read once; any S >= 1.
 *
 * tnf_ctx_flow_supported(D, S, L, U, N): 1 exactly for 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and 1 <= N <= 31;
 *   else 0.
 * tnf_ctx_flow_launch_count(which): successful calls that reached their launch, per entry; a counter space of its own
 *   (TNF_DIAG_FAMILIES is a closed set).  No tnf_diag_launch_count family moves.
 *
 * Arguments.  params (M, pstride): one row per context, the layout of tnf_flow_num_params(D, S, L, U); trailing extra
 * parameters are ignored.  bn_mean / bn_alpha (2S, D): the frozen BatchNorm statistics, shared by all contexts.  Rows need
 * 4-byte alignment only.
 *   tnf_ctx_flow_log_prob_f32  the inverse pass.  z (M_z, N, D) with M_z = 1 (one block of rows for every context) or M.
 *                              Any non-empty subset of log_prob (M, N), z0 (M, N, D) and sum_log_det (M, N) -- the summed
 *                              FORWARD log-dets, as NormFlow.inverse_and_log_det returns them -- may be asked for (NULL:
 *                              not wanted).  log_prob is the reference's float32 formula (density_estimator.py:413-416).
 *   tnf_ctx_flow_forward_f32   the sampling pass with frozen statistics.  omega (M, N, D) -> z_out (M, N, D) and the
 *                              summed forward log-det sum_log_det (M, N) (either may be NULL, not both); the caller forms
 *                              the float64 log_q = log N(omega; 0, I) - sum_log_det.
 * Refused before any launch: a NULL input, no output requested, M < 1, M_z not in {1, M}, N < 0,
 * pstride < tnf_flow_num_params(D, S, L, U), z0 == z and z_out == omega are TNF_EINVAL; a shape for which
 * tnf_ctx_flow_supported is 0 (N = 32 included) is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a launch.
 * Each successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * CTXFLOW_SIGNATURES; tests/test_ctx_flow_host.py keeps this header, the exports and that table in step.
 * float32 only; no gradients here: the backward of tnf_ctx_flow_log_prob_f32 from its z0 is tnf_ctxtrain.h. */
#ifndef TNF_CTXFLOW_H
#define TNF_CTXFLOW_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TNF_CTXFLOW_COUNT_LOG_PROB = 0, TNF_CTXFLOW_COUNT_FORWARD = 1, TNF_CTXFLOW_COUNTERS = 2 };
int tnf_ctx_flow_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_flow_launch_count(int32_t which);
int tnf_ctx_flow_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M, int64_t N, int32_t D,
                              int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream);
int tnf_ctx_flow_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                             float* z_out, float* sum_log_det, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L,
                             int32_t U, int64_t pstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_CTXFLOW_H */
