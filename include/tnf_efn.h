/* Exponential-family-network (EFN) entries of libtnf_hip.so: the prior over natural parameters (`sample_eta`,
 * exponential_families.py:116-138, 231-251 of the reference) and the per-context KL diagnostic (`KL`, :207-215, 295-307)
 * as HIP kernels, so that a whole train_efn iteration (notebooks/two_network_arch.ipynb cell 5: draw eta, sample the
 * flow, loss, backward, Adam, KL) stays on the device.  Included by tnf.h; a header of its own for the reason tnf_mog.h
 * gives.  Bound by torch_nf_amd/_lib.py EFN_SIGNATURES; tests/test_efn_host.py keeps this header, the exports and that
 * table in step.  float32 only; the families are TNF_EF_MVN / TNF_EF_DIRICHLET of tnf.h, 1 <= D <= TNF_EFN_MAX_D.
 *
 * THE STREAM is that of tnf_abc.h / tnf_hebb.h: Philox4x32-10, a pure function of (seed, t, m, k) for context m and
 * per-context draw index k = 0 .. K - 1:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (k / 4, t, i0 + m, TNF_EFN_PURPOSE_NORMAL or TNF_EFN_PURPOSE_UNIFORM)
 * The block's four words w0 .. w3 give draws 4b .. 4b + 3: normals by the Box-Muller pairs of tnf_abc.h ((w0, w1) ->
 * draws 4b, 4b + 1; (w2, w3) -> 4b + 2, 4b + 3), bit for bit; uniforms u = ((float)(w >> 8) + 0.5f) * 2^-24, one per
 * word.  t is the caller's draw index; when t_dev is non-NULL the kernels read t from that device word (int64; its low
 * 32 bits are the counter word) instead, so that a captured step advances the stream by incrementing a device tensor.
 * Nothing depends on which lane, wave or launch evaluates a context.  Limits: 0 <= t < 2^31, i0 >= 0, M >= 0,
 * i0 + M <= 2^31.
 *
 * Draw order per context.  MVN, df = iw_df_fac * D, K = D (1 + df) normals:
 *   1. k = 0 .. D - 1                      n_k, mu_k = sigma_mu * n_k
 *   2. the next D (D - 1) / 2              the strict lower triangle of the Bartlett factor L, row-major (L[i][j], i > j)
 *   3. for i = 0 .. D - 1, df - i normals  L[i][i] = sqrt(sum of their squares): a chi-square with df - i degrees of
 *                                          freedom, exact and branch-free (no rejection loop)
 *   W = L L^T / df ~ Wishart(df, I / df) IS the precision matrix: the reference draws Sigma ~ IW(df, df I) (= inv(W)) and
 *   its mu_to_eta inverts Sigma again.  Nothing is inverted here: eta = [W mu | packed row-major upper triangle with
 *   -W_ii / 2 on the diagonal and -W_ij off it] (:158-185), D_eta = D + D (D + 1) / 2.
 * Dirichlet, K = D uniforms: alpha_k = fma(ub - lb, u_k, lb), eta = [alpha | 1], D_eta = D + 1.
 *
 * tnf_efn_supported(family, D): 1 for a known family and 1 <= D <= TNF_EFN_MAX_D, else 0.
 * tnf_efn_launch_count(which): launches per entry point, a counter space of its own like tnf_hebb_launch_count.
 * tnf_efn_prior_num_noise(family, D, iw_df_fac): K, or -1 where tnf_efn_prior_f32 would refuse the three.
 * tnf_efn_prior_noise_f32: noise (M, K), exactly the normals / uniforms the prior consumes for (seed, t, i0 .. i0 + M).
 * tnf_efn_prior_f32: eta (M, D_eta).  noise NULL: the in-kernel stream; else (M, K) draws consumed in its place -- with
 *   the noise entry's output the result equals the in-kernel-stream result bit for bit.  sigma_mu and iw_df_fac are read
 *   for MVN only, lb and ub for Dirichlet only.  Checked before any launch: an unsupported (family, D) is
 *   TNF_EUNSUPPORTED; a NULL eta, iw_df_fac < 1, df > TNF_EFN_MAX_DF, a negative or NaN sigma_mu, lb > ub or either
 *   non-finite, and the stream's limits are TNF_EINVAL.  M == 0 returns TNF_OK without a launch.
 * tnf_efn_kl_f32: kl[m] = mean_n(log_q[m][n] - log p(z[m][n]; eta[m])), z (M, N, D), log_q (M, N) of log_q_dtype
 *   (TNF_F32 or TNF_F64), eta (M, D_eta) contiguous, kl (M) float32.  N >= 1.  Three launches, no float atomics, no host
 *   synchronisation:
 *   prepare  one wave per context.  MVN: P from eta (P_ii = -2 eta2_ii, P_ij = -eta2_ij), Cholesky P = C C^T in LDS,
 *            mu = P^-1 eta1 by two triangular solves; the workspace row is [mu | C^T packed row-major upper triangle |
 *            sum_i log C_ii - D/2 log 2 pi], the layout of eta plus one constant.  A pivot that is not a finite positive
 *            number makes that context's constant -- and so its kl -- NaN (numpy's Cholesky raises there); other
 *            contexts are unaffected.  Dirichlet: [alpha - 1 | lgamma(sum alpha) - sum lgamma(alpha_i)], the constant
 *            evaluated in double; an alpha that is not a positive number makes it NaN.
 *   stream   one context x a run of 128-sample tiles per workgroup.  MVN: y = C^T (z - mu), log p = -|y|^2 / 2 + const.
 *            Dirichlet: z' = (z + 1e-32) / sum(z + 1e-32), log p = const + sum (alpha_i - 1) log z'_i.  log_q - log p is
 *            accumulated in double, one partial per workgroup, in a fixed order.
 *   reduce   the partials of a context added in workgroup order, divided by N: kl is reproducible bit for bit.
 *   tnf_efn_kl_workspace_bytes = M * (G * 8 + (D_eta + 1) * 4), G <= 8192 workgroups per context a function of (M, N);
 *   -1 on bad arguments.  A NULL z / log_q / eta / kl / workspace, N < 1, M < 0 and a log_q_dtype other than the two
 *   are TNF_EINVAL, a workspace that is too small TNF_EWORKSPACE, an unsupported (family, D) TNF_EUNSUPPORTED.
 * The kernels use plain vector stores only: no atomics, no host synchronisation, no allocation. */
#ifndef TNF_EFN_H
#define TNF_EFN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TNF_EFN_MAX_D 64
#define TNF_EFN_MAX_DF 1024
#define TNF_EFN_PURPOSE_NORMAL 0x45464E00u
#define TNF_EFN_PURPOSE_UNIFORM 0x45464E01u
enum { TNF_EFN_COUNT_PRIOR = 0, TNF_EFN_COUNT_NOISE = 1, TNF_EFN_COUNT_KL = 2, TNF_EFN_COUNTERS = 3 };
int tnf_efn_supported(int32_t family, int32_t D);
int64_t tnf_efn_launch_count(int32_t which);
int64_t tnf_efn_prior_num_noise(int32_t family, int32_t D, int32_t iw_df_fac);
int tnf_efn_prior_noise_f32(float* noise, const int64_t* t_dev, int32_t family, int32_t D, int32_t iw_df_fac, int64_t seed,
                            int64_t t, int64_t i0, int64_t M, void* stream);
int tnf_efn_prior_f32(float* eta, const float* noise, const int64_t* t_dev, int32_t family, int32_t D, int32_t iw_df_fac,
                      float sigma_mu, float lb, float ub, int64_t seed, int64_t t, int64_t i0, int64_t M, void* stream);
int64_t tnf_efn_kl_workspace_bytes(int32_t family, int64_t M, int64_t N, int32_t D);
int tnf_efn_kl_f32(const float* z, const void* log_q, int32_t log_q_dtype, const float* eta, float* kl, int32_t family,
                   int64_t M, int64_t N, int32_t D, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_EFN_H */
