/* Training per-context RealNVP ("coupling") flows with 17 <= num_units <= 64 through their samples, with few samples per
 * context: the backward of tnf_ctx_wide_forward_f32 (tnf_ctxwide.h, frozen BatchNorm statistics) in one launch -- one
 * parameter row per context m and 1 <= N <= 31 draws per context, as in z, log_q = ConditionalDensityEstimator(x, N,
 * freeze_bn=True) followed by loss(z, log_q).backward(), at every width 2 <= D <= 64.  tnf_ctxsample.h covers this call
 * up to 16 units; tnf_ctxwide.h covers these widths for inference and for the backward of log_prob.
 *
 * The kernel (csrc/flow_ctx_wide_sample_bwd.hip) is the reversible walk of tnf_ctxsample.h -- from the z the forward
 * returned, bijectors last to first, each layer's input rebuilt by the inverse map, plain float32 on the real widths --
 * with the mapping of tnf_ctx_wide_log_prob_bwd_f32: one workgroup per context and up to 150 KB of dynamic LDS for the
 * context's slice.  No activations are kept between forward and backward, no prepared image, no workspace, any S >= 1.
 *
 * tnf_ctx_wide_sample_supported(D, S, L, U, N): tnf_ctx_wide_supported and tnf_ctx_wide_train_supported, both: the
 *   forward needs one layer's operand image within 150 KB of LDS, the backward the context's slice and L <= 3; else 0.
 * tnf_ctx_wide_sample_launch_count(): successful calls of the backward that reached their launch; a counter of its own
 *   (TNF_DIAG_FAMILIES and TNF_CTXWIDE_COUNTERS are closed sets; none of their counters moves, nor does
 *   tnf_ctx_sample_launch_count).
 * tnf_ctx_wide_sample_waves(D, U, N): the waves of the workgroup (4, 8 or 16) the backward chooses for a shape by itself,
 *   or -1 outside 2 <= D <= 64, 17 <= U <= 64, 1 <= N <= 31.
 * tnf_ctx_wide_sample_set_waves(waves): a process-wide override of that choice, for measurements and tests: 4, 8 or 16
 *   force a team, 0 (the default) gives the choice back; anything else is TNF_EINVAL and changes nothing.  Returns the
 *   previous value.  The results are the same bits for every team size.
 * tnf_ctx_wide_sample_bwd_f32: the arguments of tnf_ctx_sample_bwd_f32 (tnf_ctxsample.h), with z (M, N, D) as
 *   tnf_ctx_wide_forward_f32 wrote it: params (M, pstride); bn_mean / bn_alpha (2S, D); g_z (M, N, D) or NULL (zero);
 *   g_sld (M, N) or NULL (zero)
 *   -> g_params (M, gpstride): each of the tnf_flow_num_params slots of a row is written exactly once (no atomics,
 *      nothing accumulated: the rows need no initialisation); columns beyond the parameter count are not touched.
 *   -> g_omega (M, N, D), the gradient with respect to the draw through the flow; NULL: not wanted.
 *   Every sum over a context's samples is taken in a fixed order: results are bit-reproducible, and context m's outputs
 *   depend neither on the other contexts of the call nor on the team size.  Rows need 4-byte alignment only.
 * Refused before any launch, in this order: a NULL z, params, statistics pointer or g_params; g_z and g_sld both NULL;
 * M < 1 or N < 0; M > 32768 x 65535 (TNF_EINVAL); a shape for which tnf_ctx_wide_sample_supported is 0, N = 32 and
 * U = 16 included (TNF_EUNSUPPORTED); pstride or gpstride below tnf_flow_num_params(D, S, L, U); g_omega == z or
 * g_omega == g_z; g_params == params (TNF_EINVAL).  N == 0 returns TNF_OK without a launch, after every check.
 * A successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * CTXWIDESAMPLE_ENTRIES; tests/test_ctx_wide_sample_host.py keeps this header, the exports and that table in step.
 * float32 only; arch_type "coupling" only; frozen statistics only (fresh batch statistics keep their routes). */
#ifndef TNF_CTXWIDESAMPLE_H
#define TNF_CTXWIDESAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tnf_ctx_wide_sample_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N);
int64_t tnf_ctx_wide_sample_launch_count(void);
int tnf_ctx_wide_sample_waves(int32_t D, int32_t U, int64_t N);
int tnf_ctx_wide_sample_set_waves(int32_t waves);
int tnf_ctx_wide_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                                const float* g_z, const float* g_sld, float* g_params, float* g_omega, int64_t M, int64_t N,
                                int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_CTXWIDESAMPLE_H */
