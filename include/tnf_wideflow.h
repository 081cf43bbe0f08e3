/* Whole-flow RealNVP ("coupling") kernel for hidden widths 17 <= num_units <= 64 at every width 2 <= D <= 64: plain
 * log_prob, inverse_and_log_det, frozen-statistics forward and sample in ONE launch per call.  Above 16 units the
 * one-call kernels of tnf.h do not apply and these calls run the per-layer wide chain (D % 8 == 0: 2 S launches plus an
 * image and a fold kernel, z through HBM between layers) or the per-bijector composition (every other D: 5 S launches).
 * Here one workgroup owns one parameter row: it builds the folded exact-f32 MFMA operand images of all 2 S coupling
 * layers (real half widths D / 2 and D - D / 2, zero-padded to 16 or 32) and the BatchNorm / Affine maps between them in
 * LDS, straight from the packed row, then walks 16-sample tiles through all layers in registers.  No prepared images, no
 * workspace, no second launch; per-context parameter rows work because the image is built per workgroup.
 *
 * tnf_wide_flow_supported(D, S, L, U): 1 exactly for 2 <= D <= 64, S >= 1, 1 <= L <= 5, 17 <= U <= 64 and
 *   8 S (floats + 64 HT) <= 153,600 bytes of LDS, where HT = ceil(ceil(D / 2) / 16), UT = ceil(U / 16),
 *   floats = 256 (4 HT UT + 2 (L - 1) UT UT) + 16 (2 L UT + 2 HT) is one layer's operand image
 *   (csrc/wide_flow_tile.h); else 0.  At L = 2: S <= 4 for D <= 32, U <= 32; S <= 2 for D >= 33, U <= 32; S = 1 for
 *   U >= 49.  U <= 16 is not claimed: those shapes have faster split-f16 kernels.
 * tnf_wide_flow_launch_count(which): successful calls that reached their launch, per entry; a counter space of its own
 *   (TNF_DIAG_FAMILIES is a closed set).  No tnf_diag_launch_count family moves.
 *
 * Arguments.  params (M_p, pstride): the layout of tnf_flow_num_params(D, S, L, U); trailing extra parameters are
 * ignored.  bn_mean / bn_alpha (2S, D): the frozen BatchNorm statistics, shared by all rows.  Rows need 4-byte alignment
 * only.  M = max(M_z, M_p).
 *   tnf_wide_flow_log_prob_f32  the inverse pass.  z (M_z, N, D); M_z and M_p in {1, M}.  Any non-empty subset of
 *                               log_prob (M, N), z0 (M, N, D) and sum_log_det (M, N) -- the summed FORWARD log-dets, as
 *                               NormFlow.inverse_and_log_det returns them -- may be asked for (NULL: not wanted).
 *                               log_prob is the reference's float32 formula (density_estimator.py:413-416).
 *   tnf_wide_flow_forward_f32   the sampling pass with frozen statistics.  omega (M_z, N, D) with M_z = M: one block of
 *                               draws per parameter row (M_p = M) or one shared parameter row (M_p = 1).  z_out (M, N, D)
 *                               and the summed forward log-det sum_log_det (M, N) (either may be NULL, not both); the
 *                               caller forms the float64 log_q = log N(omega; 0, I) - sum_log_det.
 * Refused before any launch: a NULL input, no output requested, M_z or M_p < 1 or not in {1, M} (sampling: M_z != M),
 * N < 0, pstride < tnf_flow_num_params(D, S, L, U), z0 == z and z_out == omega are TNF_EINVAL; a shape for which
 * tnf_wide_flow_supported is 0 is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a launch.
 * Each successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * WIDEFLOW_SIGNATURES; tests/test_wideflow_host.py keeps this header, the exports and that table in step.
 * float32 only; no gradients. */
#ifndef TNF_WIDEFLOW_H
#define TNF_WIDEFLOW_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TNF_WIDEFLOW_COUNT_LOG_PROB = 0, TNF_WIDEFLOW_COUNT_FORWARD = 1, TNF_WIDEFLOW_COUNTERS = 2 };
int tnf_wide_flow_supported(int32_t D, int32_t S, int32_t L, int32_t U);
int64_t tnf_wide_flow_launch_count(int32_t which);
int tnf_wide_flow_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                               float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N,
                               int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream);
int tnf_wide_flow_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* z_out, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N, int32_t D, int32_t S,
                              int32_t L, int32_t U, int64_t pstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_WIDEFLOW_H */
