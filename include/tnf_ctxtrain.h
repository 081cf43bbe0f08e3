/* Training per-context RealNVP ("coupling") flows with few samples per context: the backward of
 * tnf_ctx_flow_log_prob_f32 (tnf_ctxflow.h) in one launch -- one parameter row per context m and 1 <= N <= 31 rows of z
 * per context, as in ConditionalDensityEstimator.log_prob(z (M, N, D), x) under autograd (lfi.train_APT's atoms, a
 * contrastive or validation loss over contexts x a few samples), at every width 2 <= D <= 64.
 *
 * The backward is reversible: it starts from the z0 that the forward kept, with g_z0 = -g_lp z0 and a log-det cotangent
 * of -g_lp, and walks the bijectors first to last (the reverse of the order log_prob evaluated them in).  At each
 * coupling layer it recomputes the twin nets from the conditioner half, rebuilds the layer's input by the
 * sampling-direction map z2 <- t + z2 e^s, sends the deltas back through the transposed weights and contracts activations
 * with deltas over the context's samples.  One wave serves one context (a whole workgroup where four contexts' slices
 * exceed 64 KB of LDS) and holds the state, its gradient, the current layer's block of the parameter row and the layer's
 * activations in its slice of LDS; the arithmetic is plain float32 on
 * the layer's real widths (h = D / 2, D - h and U: nothing is padded, so no padded row, feature or unit exists).  No
 * activations are kept between forward and backward, no prepared image, no workspace, any S >= 1.
 *
 * tnf_ctx_train_supported(D, S, L, U, N): 1 exactly for 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and
 *   1 <= N <= 31 (the domain of tnf_ctx_flow_supported); else 0.
 * tnf_ctx_train_launch_count(): successful calls of the backward that reached their launch; a counter of its own
 *   (TNF_DIAG_FAMILIES and TNF_CTXFLOW_COUNTERS are closed sets; none of their counters moves).
 * tnf_ctx_train_log_prob_bwd_f32: z0 (M, N, D) as tnf_ctx_flow_log_prob_f32 wrote it; params (M, pstride), one row per
 *   context in the layout of tnf_flow_num_params(D, S, L, U); bn_mean / bn_alpha (2S, D), the frozen BatchNorm statistics
 *   shared by all contexts (constants: no gradient); g_lp (M, N), the upstream gradient of log_prob.
 *   -> g_params (M, gpstride): each of the tnf_flow_num_params slots of a row is written exactly once, by the lanes
 *      that own the context (no atomics, nothing accumulated: the rows need no initialisation); columns beyond the
 *      parameter count are not touched.
 *   -> g_z (M, N, D), the gradient with respect to the z of log_prob; NULL: not wanted.
 *   Every sum over a context's samples is taken in a fixed order: results are bit-reproducible, and context m's outputs
 *   do not depend on which other contexts are in the call.  Rows need 4-byte alignment only.
 * Refused before any launch: a NULL input or a NULL g_params, M < 1, N < 0, pstride or gpstride below
 * tnf_flow_num_params(D, S, L, U), g_z == z0 and g_params == params are TNF_EINVAL; a shape for which
 * tnf_ctx_train_supported is 0 (N = 32 included) is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a launch.
 * A successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * CTXTRAIN_SIGNATURES; tests/test_ctx_train_host.py keeps this header, the exports and that table in step.
 * float32 only; log_prob only (no gradients through the sampling direction). */
#ifndef TNF_CTXTRAIN_H
#define TNF_CTXTRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tnf_ctx_train_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_train_launch_count(void);
int tnf_ctx_train_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                   const float* g_lp, float* g_params, float* g_z, int64_t M, int64_t N, int32_t D,
                                   int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_CTXTRAIN_H */
