/* Per-context RealNVP ("coupling") flows with 17 <= num_units <= 64 and few samples per context, one launch per call each
 * way: one parameter row per context m and 1 <= N <= 31 rows of z per context -- ConditionalDensityEstimator.log_prob(
 * z (M, N, D), x), cde(x, N, freeze_bn=True), cde.sample(x, N) and log_prob under autograd -- at every width
 * 2 <= D <= 64.  tnf_ctxflow.h / tnf_ctxtrain.h cover this layout up to 16 units; tnf_wideflow.h covers these widths
 * for many samples per row, with the operand images of all 2 S layers resident (S <= 4 .. 1) and no gradients.
 *
 * Inference (csrc/flow_ctx_wide.hip).  One workgroup serves one context.  The context's one or two 16-sample tiles stay
 * in registers for the whole flow, and the workgroup walks the 2 S coupling layers ONE LAYER AT A TIME: all its waves
 * build the layer's folded exact-f32 MFMA operand image (csrc/wide_flow_tile.h) and the layer's BatchNorm / Affine fold
 * block in LDS straight from the context's packed row, the tile-holding waves run the layer, and the next layer's image
 * replaces it.  Only one image is resident, so S is unbounded.  No prepared images, no workspace, no second launch.
 *
 * Training (csrc/flow_ctx_wide_bwd.hip).  The backward of tnf_ctx_wide_log_prob_f32 from its z0 in one launch: the
 * reversible walk of tnf_ctxtrain.h (csrc/ctx_bwd_walk.h: plain float32 on the real widths, every gradient slot written
 * once, no atomics, no workspace) with one workgroup per context and up to 150 KB of LDS for the context's slice.
 *
 * Both need 2 <= D <= 64, S >= 1, 17 <= U <= 64 and 1 <= N <= 31 (the domain); then
 * tnf_ctx_wide_lds_bytes(which, D, S, L, U, N): the dynamic LDS of one workgroup, for any L >= 1; -1 outside the domain
 *   or for another `which`.
 *     which = 0, the inference launch: 4 (floats + 64 HT) with HT = ceil(ceil(D / 2) / 16), UT = ceil(U / 16) and
 *       floats = 256 (4 HT UT + 2 (L - 1) UT UT) + 16 (2 L UT + 2 HT), one layer's operand image and its fold block
 *       (independent of S and N).
 *     which = 1, the backward launch: 4 ceil4(2 N D + N + wb + 2 L N U + 2 N (D - D / 2)), the slice of
 *       csrc/ctx_bwd_walk.h, where wb is the larger of a stage's two coupling blocks, the lower one with its 2 D Affine
 *       parameters, and ceil4 rounds up to a multiple of 4.
 * tnf_ctx_wide_supported(D, S, L, U, N): 1 exactly in the domain with 1 <= L <= 5 and lds_bytes(0, ...) <= 153,600: all
 *   of L <= 4, and L = 5 but D >= 33 with U >= 49; else 0.
 * tnf_ctx_wide_train_supported(D, S, L, U, N): 1 exactly in the domain with 1 <= L <= 3 and lds_bytes(1, ...) <=
 *   153,600: all of L <= 2, all of L = 3 with U <= 48, and L = 3 above 48 units where D x N is small enough (D = 64,
 *   U = 64: N <= 22); else 0.
 *   N = 32 and U = 16 are outside the domain of both.
 * tnf_ctx_wide_launch_count(which): successful calls that reached their launch, per entry; a counter space of its own
 *   (TNF_DIAG_FAMILIES, TNF_CTXFLOW_COUNTERS and TNF_WIDEFLOW_COUNTERS are closed sets; none of their counters, nor
 *   tnf_ctx_train_launch_count, moves).
 *
 * Arguments.  params (M, pstride): one row per context, the layout of tnf_flow_num_params(D, S, L, U); trailing extra
 * parameters are ignored.  bn_mean / bn_alpha (2S, D): the frozen BatchNorm statistics, shared by all contexts
 * (constants: no gradient).  Rows need 4-byte alignment only.
 *   tnf_ctx_wide_log_prob_f32      the inverse pass; arguments and refusals of tnf_ctx_flow_log_prob_f32.  z (M_z, N, D)
 *                                  with M_z = 1 (one block of rows for every context) or M.  Any non-empty subset of
 *                                  log_prob (M, N), z0 (M, N, D) and sum_log_det (M, N) -- the summed FORWARD log-dets --
 *                                  may be asked for (NULL: not wanted).  log_prob is the reference's float32 formula
 *                                  (density_estimator.py:413-416).
 *   tnf_ctx_wide_forward_f32       the sampling pass with frozen statistics; arguments and refusals of
 *                                  tnf_ctx_flow_forward_f32.  omega (M, N, D) -> z_out (M, N, D) and the summed forward
 *                                  log-det sum_log_det (M, N) (either may be NULL, not both).
 *   tnf_ctx_wide_log_prob_bwd_f32  arguments and refusals of tnf_ctx_train_log_prob_bwd_f32.  z0 (M, N, D) as
 *                                  tnf_ctx_wide_log_prob_f32 wrote it, g_lp (M, N) -> g_params (M, gpstride): each of the
 *                                  tnf_flow_num_params slots of a row is written exactly once (the rows need no
 *                                  initialisation; columns beyond the parameter count are not touched), and g_z
 *                                  (M, N, D) or NULL.  Every sum over a context's samples is taken in a fixed order:
 *                                  bit-reproducible, and context m's outputs do not depend on the other contexts.
 * Refused before any launch: a NULL input (g_params included), no output requested, M < 1, M_z not in {1, M}, N < 0,
 * pstride or gpstride below tnf_flow_num_params(D, S, L, U), z0 == z, z_out == omega, g_z == z0 and g_params == params
 * are TNF_EINVAL; a shape for which the entry's predicate is 0 is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a
 * launch.  Each successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * CTXWIDE_SIGNATURES; tests/test_ctx_wide_host.py keeps this header, the exports and that table in step.
 * float32 only; arch_type "coupling" only; no gradients through the sampling direction, no fresh statistics. */
#ifndef TNF_CTXWIDE_H
#define TNF_CTXWIDE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    TNF_CTXWIDE_COUNT_LOG_PROB = 0,
    TNF_CTXWIDE_COUNT_FORWARD = 1,
    TNF_CTXWIDE_COUNT_LOG_PROB_BWD = 2,
    TNF_CTXWIDE_COUNTERS = 3
};
int tnf_ctx_wide_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int tnf_ctx_wide_train_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_wide_lds_bytes(int32_t which, int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_wide_launch_count(int32_t which);
int tnf_ctx_wide_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M, int64_t N, int32_t D,
                              int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream);
int tnf_ctx_wide_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                             float* z_out, float* sum_log_det, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L,
                             int32_t U, int64_t pstride, void* stream);
int tnf_ctx_wide_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                  const float* g_lp, float* g_params, float* g_z, int64_t M, int64_t N, int32_t D,
                                  int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_CTXWIDE_H */
