/* Training per-context RealNVP ("coupling") flows through their samples, with few samples per context: the backward of
 * tnf_ctx_flow_forward_f32 (tnf_ctxflow.h, frozen BatchNorm statistics) in one launch -- one parameter row per context m
 * and 1 <= N <= 31 draws per context, as in z, log_q = ConditionalDensityEstimator(x, N, freeze_bn=True) followed by
 * loss(z, log_q).backward() (amortised variational inference, an EFN step with a handful of draws per context), at every
 * width 2 <= D <= 64.
 *
 * The backward is reversible: it starts from the z that the forward returned, with the upstream gradients g_z and g_sld
 * (the cotangent of the summed log-det), and walks the bijectors last to first (the reverse of the order the sampling
 * pass evaluated them in): per stage the Affine block, BatchNorm c1, the lower coupling layer, BatchNorm c0, the upper
 * coupling layer.  At each coupling layer it recomputes the twin nets from the conditioner half, rebuilds the layer's
 * input by the inverse map x2 <- (y2 - t) e^-s, sends the deltas back through the transposed weights and contracts
 * activations with deltas over the context's samples.  One wave serves one context (a whole workgroup where four
 * contexts' slices exceed 64 KB of LDS) and holds the state, its gradient, the current layer's block of the parameter row
 * and the layer's activations in its slice of LDS; the arithmetic is plain float32 on the layer's real widths (h = D / 2,
 * D - h and U: nothing is padded, so no padded row, feature or unit exists).  No activations are kept between forward and
 * backward, no prepared image, no workspace, any S >= 1.
 *
 * tnf_ctx_sample_supported(D, S, L, U, N): 1 exactly for 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and
 *   1 <= N <= 31 (the domain of tnf_ctx_train_supported and tnf_ctx_flow_supported); else 0.
 * tnf_ctx_sample_launch_count(): successful calls of the backward that reached their launch; a counter of its own
 *   (TNF_DIAG_FAMILIES and TNF_CTXFLOW_COUNTERS are closed sets; none of their counters moves, nor does
 *   tnf_ctx_train_launch_count).
 * tnf_ctx_sample_bwd_f32: z (M, N, D) as tnf_ctx_flow_forward_f32 wrote it; params (M, pstride), one row per context in
 *   the layout of tnf_flow_num_params(D, S, L, U); bn_mean / bn_alpha (2S, D), the frozen BatchNorm statistics shared by
 *   all contexts (constants: no gradient); g_z (M, N, D), the upstream gradient of z, or NULL (zero); g_sld (M, N), the
 *   upstream gradient of the forward's summed log-det, or NULL (zero) -- a caller that forms
 *   log_q = log N(omega; 0, I) - sum_log_det passes g_sld = -g_log_q.
 *   -> g_params (M, gpstride): each of the tnf_flow_num_params slots of a row is written exactly once, by the lanes
 *      that own the context (no atomics, nothing accumulated: the rows need no initialisation); columns beyond the
 *      parameter count are not touched.
 *   -> g_omega (M, N, D), the gradient with respect to the draw through the flow (the base density's own term is the
 *      caller's); NULL: not wanted.
 *   Every sum over a context's samples is taken in a fixed order: results are bit-reproducible, and context m's outputs
 *   do not depend on which other contexts are in the call.  Rows need 4-byte alignment only.
 * Refused before any launch: a NULL z, params, statistics pointer or g_params, g_z and g_sld both NULL, M < 1,
 * M > 2^31 - 1, N < 0, pstride or gpstride below tnf_flow_num_params(D, S, L, U), g_omega == z or g_omega == g_z and
 * g_params == params are TNF_EINVAL; a shape for which tnf_ctx_sample_supported is 0 (N = 32 included) or whose slice
 * exceeds 64 KB is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a launch.
 * A successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * CTXSAMPLE_SIGNATURES; tests/test_ctx_sample_host.py keeps this header, the exports and that table in step.
 * float32 only; frozen statistics only (fresh batch statistics keep their routes). */
#ifndef TNF_CTXSAMPLE_H
#define TNF_CTXSAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tnf_ctx_sample_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_sample_launch_count(void);
int tnf_ctx_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                           const float* g_z, const float* g_sld, float* g_params, float* g_omega, int64_t M, int64_t N,
                           int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_CTXSAMPLE_H */
