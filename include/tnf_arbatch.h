/* Sampling an autoregressive flow -- NormFlow(arch_type="AR") = [MAF, BatchNorm, Affine] -- with FRESH batch statistics
 * as one call each way: what nf(N), cde(x, N) and cde.sample(eta, N, freeze_bn=False) run, and what every iteration of
 * efn.train_efn differentiates.  Layout as in tnf_arsample.h: params (M_p, pstride) = [MAF | a (D) | b (D)], M_p is 1 or
 * M; the statistics are taken over all M * N rows (bijectors.py:401-417).  float32, exact-f32 MFMA operands.
 *
 * Forward, at most four kernels (and one memset):
 *   1. x = MAF_fwd(omega), sum_log_det = A(x): the matrix-pipe MAF kernel of tnf_maf, without a fold behind it;
 *   2. the double moments [sum x | sum x^2] over the M * N rows (the streaming pass of tnf_bn_batch_moments_f32);
 *   3. one workgroup per parameter row: mean = sum / n, alpha = sqrt(max(var_b, 0) + eps) in double, cast to float,
 *      fold A = e^a / alpha, B = b - mean A, ldc = sum a - sum log alpha (the statements of the coupling chains' fold);
 *   4. in place z = x A + B, sum_log_det += ldc (float4 accesses when D % 4 == 0 and z_out is 16-byte aligned).
 * Backward, at most four kernels.  With n = M N, y = (z - b) e^-a, P_d = sum g_z e^a, Q_d = sum g_z (z - b),
 * G = sum g_sld over ALL rows:
 *   1. per workgroup (a fixed slice of one context's rows, added in row order) the double partials of
 *      GZ = sum g_z z, GB = sum g_z, GS = sum g_sld;
 *   2. one workgroup adds the partials in a fixed order into P, Q, G (and the totals of a shared row), all double;
 *   3. per parameter row: g_a = GZ - b GB + GS and g_b = GB are ADDED to the Affine slice of g_params, and the rows
 *      A' = alpha e^-a, B' = mean - b A', C0 = e^a / alpha, C2 = -e^-a (Q + G) / (n alpha), C1 = -P / (n alpha) - b C2
 *      are written: x = z A' + B' and g_x = g_z C0 + C1 + z C2 -- the composition of tnf_affine_backward and
 *      tnf_bn_batch_backward_f32 with G the cotangent of BatchNorm's 0-dim log-det;
 *   4. the walk of tnf_maf_sample_bwd_f32 at (x, g_x, g_ld = g_sld), whose load stage forms x and g_x from z and g_z.
 * No atomics in 1 .. 3: P, Q, G and the Affine slice are bit-reproducible from call to call.  The MAF block of g_params
 * follows tnf_arsample.h: the caller zeroes g_params; per-context rows are written, one shared row is flushed by atomics.
 * Nothing is kept between the two calls but z and the 2 D statistics.
 *
 * tnf_ar_flow_batch_supported(D, L, U): the forward's domain, that of tnf_ar_flow_supported.
 * tnf_ar_flow_batch_train_supported(D, L, U): tnf_ar_flow_supported and tnf_maf_sample_bwd_supported (D <= 32, L <= 3,
 *   U <= 64).
 * tnf_arbatch_launch_count(which): TNF_ARBATCH_COUNT_FWD_CALLS / _BWD_CALLS: calls of the entry that reached a launch;
 *   _FWD_KERNELS / _BWD_KERNELS: kernels those calls launched.  TNF_EINVAL for another `which`.
 * tnf_ar_flow_forward_batch_workspace_bytes(M, M_p, N, D) / tnf_ar_flow_batch_bwd_workspace_bytes(M, M_p, N, D): the
 *   workspaces, 16-byte aligned; TNF_EINVAL for M < 1, M_p not in {1, M}, N < 0, D < 1 or (backward) D > 32.
 * tnf_ar_flow_forward_batch_f32: omega (M, N, D) -> z_out (M, N, D) (must not be omega), sum_log_det (M, N),
 *   bn_mean_out / bn_alpha_out (D): the statistics BatchNorm caches.
 * tnf_ar_flow_batch_bwd_f32: z, bn_mean, bn_alpha as the forward wrote them; g_z (M, N, D) and g_sld (M, N), either may
 *   be NULL (= zero), not both -> g_params (M_p, gpstride).  The float4 loads of the walk are taken when D % 4 == 0 and
 *   z and g_z (if given) are 16-byte aligned, as in tnf_arsample.h.
 * Refused before any launch: a NULL required pointer, both cotangents NULL, M < 1, M_p not in {1, M}, N < 0, pstride or
 * gpstride below the row length, g_params == params, z_out == omega, M * N < 2 (with N > 0) are TNF_EINVAL; an
 * unsupported shape is TNF_EUNSUPPORTED; a NULL, short or misaligned workspace is TNF_EWORKSPACE.  N == 0 returns TNF_OK
 * without a launch.  The calls do not allocate and do not synchronise, so they can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * ARBATCH_SIGNATURES; tests/test_arbatch_host.py keeps this header, the exports and that table in step. */
#ifndef TNF_ARBATCH_H
#define TNF_ARBATCH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    TNF_ARBATCH_COUNT_FWD_CALLS = 0,
    TNF_ARBATCH_COUNT_FWD_KERNELS = 1,
    TNF_ARBATCH_COUNT_BWD_CALLS = 2,
    TNF_ARBATCH_COUNT_BWD_KERNELS = 3,
    TNF_ARBATCH_COUNTERS = 4
};

int tnf_ar_flow_batch_supported(int32_t D, int32_t L, int32_t U);
int tnf_ar_flow_batch_train_supported(int32_t D, int32_t L, int32_t U);
int64_t tnf_arbatch_launch_count(int32_t which);
int64_t tnf_ar_flow_forward_batch_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D);
int tnf_ar_flow_forward_batch_f32(const float* omega, const float* params, const float* masks, float* z_out,
                                  float* sum_log_det, float* bn_mean_out, float* bn_alpha_out, int64_t M, int64_t M_p,
                                  int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, float eps, void* workspace,
                                  int64_t workspace_bytes, void* stream);
int64_t tnf_ar_flow_batch_bwd_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D);
int tnf_ar_flow_batch_bwd_f32(const float* z, const float* params, const float* masks, const float* bn_mean,
                              const float* bn_alpha, const float* g_z, const float* g_sld, float* g_params, int64_t M,
                              int64_t M_p, int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                              void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_ARBATCH_H */
