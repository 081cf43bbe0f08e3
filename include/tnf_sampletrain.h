/* Training a RealNVP ("coupling") flow THROUGH ITS SAMPLES with frozen BatchNorm statistics: the backward of
 *   (z, sum_log_det) = tnf_flow_forward_f32 / tnf_flow_padded_forward_f32 (omega, params)
 * in one walk kernel -- z, log_q = nf.sample(N) or nf(N, freeze_bn=True) of the reference (density_estimator.py:358-388,
 * bijectors.py:397-399), then loss(z, log_q).backward(): the reparameterised objective of variational inference.  The
 * sibling of tnf_flow_log_prob_bwd_rev_f32 for the other direction, at D = 32 / 64 directly and at every other width
 * 2 <= D <= 63 at the embedded width 2H of tnf_padtrain.h.
 *
 * The flow is invertible, so nothing is kept by the forward but its output z.  The walk starts from
 *   v = z,  g = g_z = d loss / d z,  gamma = g_sld = d loss / d sum_log_det   (log_q = base(omega) - sum_log_det puts
 *                                                                              the sign into gamma by itself)
 * and meets the coupling layers last to first, c = 2S-1 .. 0.  Behind layer c the sampling pass applies the constant
 * map y = (x - B)/A (BatchNorm with the frozen statistics; on odd c also the Affine, y = e^a x + b, log_det = sum a:
 * bijectors.py:277-318), A = alpha_bn / e^a, B = mean_bn - b A.  One step:
 *   fold     x = A v + B,  g <- g / A;  with an Affine  dA = -sum_n g_y y / A,  dB = -sum_n g_y / A, and from those
 *            g_a = -A dA + b A dB + sum_n gamma,  g_b = -A dB.  The kernel keeps the sums before their division,
 *            GA = sum_n g_y y and GB = sum_n g_y, so that g_a = GA - b GB + sum_n gamma and g_b = GB hold whatever the
 *            size of A (a fixed-point sum of g_y / A would lose bits with 1/A and have the loss multiplied by A again)
 *   layer    (t, s) recomputed from the conditioner half (which the layer leaves unchanged);
 *            x2 = (v2 - t) e^-s;   d_t = g2,  d_s = g2 (v2 - t) + gamma,  g2 <- g2 e^s;
 *            (d_t, d_s) go back through the transposed weights into the conditioner half's gradient, and activations
 *            are contracted with deltas over the samples into the weight and bias gradients.
 * The state the walk ends on is the base draw omega (omega_out).  The arithmetic is that of the sibling: split-f16
 * contractions with fp32 accumulate, both cotangents pre-scaled by the power of two that brings the larger of max |g_z|
 * and max |g_sld| into [1, 2), 32-bit fixed-point accumulators with a budget of 2^13 per accumulated term in those
 * units, partial rows per workgroup added in workgroup order in 64-bit integers: g_params is bit-reproducible from call
 * to call.  A term beyond the budget (or a NaN / inf) sets *overflow and the gradient rows come back NaN, never a
 * wrapped sum.
 *
 * tnf_flow_sample_train_supported(D, S, L, U): 1 exactly where tnf_flow_train_rev_supported(D, S, L, U) is 1
 *   (D = 32, 64) or tnf_flow_padded_train_supported(D, S, L, U) is 1 (2 <= D <= 63, D != 32); else 0.
 * tnf_flow_sample_train_workspace_bytes: the workspace of the call below (at a padded width: the embedded z, g_z and
 *   omega rows, parameter and gradient rows, statistics, and the walk's own workspace at width 2H).  TNF_EINVAL for
 *   M < 1, M_p not in {1, M}, N < 0; TNF_EUNSUPPORTED for an unsupported shape.
 * tnf_sampletrain_launch_count(): successful calls that reached the walk kernel's launch; a counter of its own
 *   (TNF_DIAG_FAMILIES and TNF_PADTRAIN_COUNTERS are closed sets; the embed / gather kernels a padded call runs count
 *   in tnf_padtrain_launch_count as always).
 * tnf_flow_sample_bwd_f32: z (M, N, D), the sampling output; params (M_p, pstride) in the layout of
 *   tnf_flow_num_params(D, S, L, U); bn_mean / bn_alpha (2S, D), the frozen statistics (constants: no gradient);
 *   g_z (M, N, D) and g_sld (M, N), the two cotangents -- either may be NULL (= zero), not both.
 *   -> g_params (M_p, gpstride).  M_p is 1 or M; with M_p == 1 the M * N rows are one batch.  At D = 32 / 64 the
 *      gradient is ACCUMULATED into g_params (the caller zeroes it), as tnf_flow_log_prob_bwd_rev_f32 does; at a padded
 *      width the real row is WRITTEN over, as tnf_flow_padded_log_prob_bwd_f32 does.
 *   -> omega_out (M, N, D), the rebuilt base draw; NULL: not wanted.  It costs one row store and localises a fault: a
 *      right omega with a wrong gradient points at the deltas.
 *   -> *overflow (device int32, may be NULL): 1 when the budget did not hold.
 *   At a padded width the one call embeds z, g_z, the parameter rows and the statistics into the workspace, runs the
 *   walk at 2H, and gathers g_params and omega_out, all on `stream` (g_sld needs no embedding).  At D = 32 / 64 z, g_z
 *   and omega_out must be 16-byte aligned; the workspace always.
 * Refused before any launch: a NULL z / params / bn_mean / bn_alpha / g_params, g_z and g_sld both NULL, M < 1, M_p not
 * in {1, M}, N < 0, pstride or gpstride below tnf_flow_num_params(D, S, L, U), g_params == params and omega_out == z
 * are TNF_EINVAL; an unsupported shape is TNF_EUNSUPPORTED; a NULL or short workspace is TNF_EWORKSPACE.  N == 0
 * returns TNF_OK without a launch.  The call does not allocate and does not synchronise, so it can be captured into a
 * HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * SAMPLETRAIN_SIGNATURES; tests/test_sample_train_host.py keeps this header, the exports and that table in step.
 * float32 only; frozen statistics only (fresh ones: tnf_flow_forward_train_*); num_units <= 16. */
#ifndef TNF_SAMPLETRAIN_H
#define TNF_SAMPLETRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tnf_flow_sample_train_supported(int32_t D, int32_t S, int32_t L, int32_t U);
int64_t tnf_flow_sample_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U);
int64_t tnf_sampletrain_launch_count(void);
int tnf_flow_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                            const float* g_z, const float* g_sld, float* g_params, float* omega_out, int64_t M, int64_t M_p,
                            int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                            void* workspace, int64_t workspace_bytes, int32_t* overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_SAMPLETRAIN_H */
