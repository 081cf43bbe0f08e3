/* Training an autoregressive flow -- NormFlow(arch_type="AR") = [MAF, BatchNorm, Affine], the reference's default
 * architecture -- THROUGH ITS SAMPLES: the backward of MAF.forward_and_log_det (D - 1 sequential passes in the reference,
 * bijectors.py:742-756) in ONE kernel, and the same kernel for the whole stack with frozen BatchNorm statistics.  This is
 * what z, log_q = nf.sample(N), nf(N) or cde(x, N, freeze_bn=True) followed by loss(z, log_q).backward() differentiates.
 *
 * The sample x solves G(x, theta) = omega with G the one-pass inverse map, G(x)_d = (x_d - mu_d(x)) e^-alpha_d(x), and
 * the forward log-det is A(x) = sum_d alpha_d(x).  With K(g_out, g_ld) the backward of the inverse direction
 * (tnf_maf_backward), the kernel evaluates the nets once per 16-sample tile, iterates
 *   v <- e^alpha g_x;   D - 1 times  v <- e^alpha (g_x - N(v)),   N(v) = the nets' share of K_z(v, -g_ld)
 * in registers (deltas only: no weight gradients; N is strictly triangular in the autoregressive order, so the iteration
 * is exact after D - 1 sweeps), and ends with one full backward pass at (x; v, -g_ld):  g_omega = v,
 * g_params = -K_theta.  The route it replaces (tnf_maf_inverse_alpha, D + 1 tnf_maf_backward calls and about 3 D
 * elementwise operations) computes the same values.  float32 with exact-f32 MFMA operands; plain float accumulators.
 *
 * tnf_maf_sample_bwd_supported(D, L, U): 1 for D <= 32, L <= 3, U <= 64 with operands and accumulators within 156 KB of
 *   LDS (the domain of the matrix-pipe MAF backward), else 0.  The masks must be those of a forward-factored MADE
 *   (mu_d, alpha_d depend on x_{<d} only), as NormFlow builds them.
 * tnf_arsample_launch_count(): successful calls of the two entries below that reached the kernel launch.
 * tnf_maf_sample_bwd_f32: x (M, N, D), the sample the forward returned; params (M_p, pstride) in the layout of
 *   tnf_maf_num_params(D, L, U); masks as tnf_maf takes them; g_x (M, N, D) and g_ld (M, N), the cotangents of the sample
 *   and of the log-det -- either may be NULL (= zero), not both.
 *   -> g_omega (M, N, D), the gradient w.r.t. the base draw; NULL: not wanted.
 *   -> g_params (M_p, gpstride): the caller zeroes it, in every case.  With one shared row (M_p = 1) everything is
 *   ADDED to what is there (atomics).  With per-context rows (M_p = M > 1) the MAF block is WRITTEN (plain stores; what
 *   was there is lost) and the Affine slice of the stack entry below is ADDED (its finalize kernel).
 *   M_p is 1 or M.  Per-context rows run one workgroup per context for any N >= 1 and write each gradient once.  They
 *   are bit-reproducible from call to call where four private accumulator copies fit the LDS (maf_bwd_nacc == 4: each
 *   wave adds its tiles in a fixed order, the flush adds the four copies in wave order).  Where only one shared copy
 *   fits, the four waves add into it with LDS float atomics, whose order is not fixed once N > 16 (a second wave has a
 *   tile): not bit-reproducible.  One shared row is walked by a persistent grid and flushed through atomics: not
 *   bit-reproducible from call to call either.
 *   Alignment: every pointer is float-aligned.  The float4 loads and stores are taken only when D % 4 == 0 AND x, g_x (if
 *   given) and g_omega (if given) are 16-byte aligned; otherwise the call runs the scalar-access instantiation -- the
 *   same values, a slower load stage.  The same holds for z and g_z of the stack entry.
 * tnf_ar_flow_sample_bwd_workspace_bytes(M_p, D): the workspace of the call below (fold | fold sums).  TNF_EINVAL for
 *   M_p < 1 or D < 1.
 * tnf_ar_flow_sample_bwd_f32: the stack with frozen statistics, z = e^a (x - mean_bn) / alpha_bn + b,
 *   sum_log_det = A(x) - sum log alpha_bn + sum a.  z (M, N, D), the stack's output -- nothing else is kept by the
 *   forward; params (M_p, pstride) = [MAF | a (D) | b (D)]; bn_mean / bn_alpha (D), constants; g_z (M, N, D) and g_sld
 *   (M, N), either may be NULL, not both.  The kernel rebuilds x = z A + B (A = alpha_bn e^-a, B = mean_bn - b A), forms
 *   g_x = g_z / A and reduces GZ = sum_n g_z z, GB = sum_n g_z, GS = sum_n g_sld per parameter row; a small finalize
 *   kernel adds g_a = GZ - b GB + GS and g_b = GB.  -> g_params (M_p, gpstride), zeroed by the caller, as above.  The workspace
 *   must be 16-byte aligned.
 * Refused before any launch: a NULL required pointer, both cotangents NULL, M < 1, M_p not in {1, M}, N < 0, pstride or
 * gpstride below the row length, g_params == params are TNF_EINVAL; an unsupported shape is TNF_EUNSUPPORTED; a NULL or
 * short workspace is TNF_EWORKSPACE.  N == 0 returns TNF_OK without a launch.  The calls do not allocate and do not
 * synchronise, so they can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * ARSAMPLE_SIGNATURES; tests/test_arsample_host.py keeps this header, the exports and that table in step. */
#ifndef TNF_ARSAMPLE_H
#define TNF_ARSAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int tnf_maf_sample_bwd_supported(int32_t D, int32_t L, int32_t U);
int64_t tnf_arsample_launch_count(void);
int tnf_maf_sample_bwd_f32(const float* x, const float* params, const float* masks, const float* g_x, const float* g_ld,
                           float* g_omega, float* g_params, int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t L,
                           int32_t U, int64_t pstride, int64_t gpstride, void* stream);
int64_t tnf_ar_flow_sample_bwd_workspace_bytes(int64_t M_p, int32_t D);
int tnf_ar_flow_sample_bwd_f32(const float* z, const float* params, const float* masks, const float* bn_mean,
                               const float* bn_alpha, const float* g_z, const float* g_sld, float* g_params, int64_t M,
                               int64_t M_p, int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                               void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_ARSAMPLE_H */
