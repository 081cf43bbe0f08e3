/* Rejection-ABC entries of libtnf_hip.so: the ABC-SMC / ABC-MCMC baselines of the reference's LFI comparison
 * (scripts/smcabc_mat.py, notebooks/ABC-MCMC.ipynb cells 2, 3, 7) on one fused kernel.  Included by tnf.h; a header of
 * its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py ABC_SIGNATURES; tests/test_abc_host.py keeps
 * this header, the exports and that table in step.  float32 only.
 *
 * A TRIAL of chain i in round t, index j: omega (D standard normals), z = mu + L omega (L = chol, lower triangle,
 * row-major (D, D); z_r = mu_r + sum_{k <= r} L_rk omega_k, added in the order k = 0 .. r), accepted when
 *   bounds[0][r] < z_r < bounds[1][r] for every r                                                    (strict), and
 *   |det A(z) - x0[0]| < eps[t][0]  and  |trace A(z) - x0[1]| < eps[t][1]            (strict; the SMC entry only),
 * A(z) the symmetric d x d matrix filled row-wise from its D = d (d + 1) / 2 upper-triangle entries (systems.Mat).
 * det is by LU with partial pivoting in float32.  The round's result is the FIRST accepted trial in the order
 * j = 0, 1, 2, ...; it becomes mu of the chain's next round.  A comparison with a NaN is false: a NaN never accepts.
 *
 * The random stream is counter-based, Philox4x32-10 (Salmon et al., SC 2011), a pure function of (seed, t, i, j, k):
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (j, t, i, b)            b = k / 4, the 4-word block that holds normal k of the trial
 *   words (w0, w1) of the block -> normals 4b, 4b + 1;  (w2, w3) -> normals 4b + 2, 4b + 3, by Box-Muller:
 *     u1 = ((w >> 8) + 0.5) 2^-24,  u2 = (w' >> 8) 2^-24,  (n, n') = sqrt(-2 ln u1) (cos, sin)(2 pi u2)
 *   in float32: u1 = (float(w >> 8) + 0.5f) * 2^-24 (the sum rounds to even from 2^23 on; u1 in (0, 1]).
 * Nothing depends on which lane, wave or launch evaluates a trial; tnf_abc_propose_f32 uses t = 0 and i = the draw.
 *
 * tnf_abc_supported(d): 1 for 2 <= d <= TNF_ABC_MAX_SMC_D (D <= TNF_ABC_MAX_D = 21), else 0.
 * tnf_abc_launch_count(which): launches of the three kernels, a counter space of its own like tnf_mog_launch_count.
 * tnf_abc_smc_mat_f32: N independent chains, T rounds, ONE launch.  z0 (N, D) the starting points, chol (D, D),
 *   bounds (2, D) = [lb | ub], x0 (2) = (det, trace) observed, eps (T, 2); omega NULL (in-kernel stream) or
 *   (T, N, max_trials, D) standard normals, trial j of (t, i) using omega[t, i, j].  Out: zs (T, N, D), xs (T, N, 2) the
 *   accepted candidate's (det, trace) as the kernel computed it, trials (T, N) int32 the 1-based index of the accepted
 *   trial -- 0 if none of the round's max_trials trials was accepted; that chain's zs / xs rows are NaN and its trials 0
 *   from that round on.  Limits: 1 <= max_trials <= TNF_ABC_MAX_TRIALS = 2^24, N < 2^24, T < 2^31.
 * tnf_abc_propose_f32: the truncated-Gaussian draw alone (the box test only): mu (M_mu, D), M_mu in {1, M},
 *   1 <= D <= 21; omega NULL or (M, max_trials, D); z (M, D), trials (M) int32 as above (a draw that found no point
 *   inside the box has a NaN row and trials 0).  M < 2^24.
 * tnf_abc_noise_f32: omega[a, c, k] = normal k of trial j0 + c of chain i0 + a in round t, (n_i, n_j, D): exactly the
 *   normals the other two entries consume.  i0 + n_i <= 2^24, j0 + n_j <= 2^24, 0 <= t < 2^31.
 * N == 0, M == 0 or an empty noise block return TNF_OK without a launch. */
#ifndef TNF_ABC_H
#define TNF_ABC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TNF_ABC_MAX_D 21
#define TNF_ABC_MAX_SMC_D 6
#define TNF_ABC_MAX_TRIALS 16777216
enum { TNF_ABC_COUNT_SMC = 0, TNF_ABC_COUNT_PROPOSE = 1, TNF_ABC_COUNT_NOISE = 2, TNF_ABC_COUNTERS = 3 };
int tnf_abc_supported(int32_t d);
int64_t tnf_abc_launch_count(int32_t which);
int tnf_abc_smc_mat_f32(const float* z0, const float* chol, const float* bounds, const float* x0, const float* eps,
                        const float* omega, float* zs, float* xs, int32_t* trials, int64_t seed, int64_t N, int64_t T,
                        int32_t d, int32_t max_trials, void* stream);
int tnf_abc_propose_f32(const float* mu, const float* chol, const float* bounds, const float* omega, float* z,
                        int32_t* trials, int64_t seed, int64_t M, int64_t M_mu, int32_t D, int32_t max_trials, void* stream);
int tnf_abc_noise_f32(float* omega, int64_t seed, int64_t t, int64_t i0, int64_t n_i, int64_t j0, int64_t n_j, int32_t D,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_ABC_H */
