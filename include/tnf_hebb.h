/* Hebbian learning-rule simulator entries of libtnf_hip.so: `hebb` of the reference's notebooks/LFI_learning_rules.ipynb
 * (cell 8) on one HIP kernel, so that a whole train_nde iteration (draw, simulate, log_prob, backward, Adam) stays on the
 * device.  Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * HEBB_SIGNATURES; tests/test_hebb_host.py keeps this header, the exports and that table in step.  float32 only.
 *
 * A SIMULATION i has parameters z[i] = (alpha, beta, theta_x, b) and a state w (n neurons) that starts at its w0 row.
 * Step s = 0 .. n_steps - 1 has the global index g = j0 + s and uses row g mod N_x of the shared inputs x (N_x, n);
 * the notebook's two passes are n_steps = 2 N_x, j0 = 0.  Per step, every operation rounded to float32 on its own:
 *   y   = sum_k w_k x[g mod N_x][k]                      (any association, FMA allowed: the only freedom)
 *   dw  = alpha*y*(x_k - theta_x) - beta*(y*y)*w_k       ((alpha*y)*(x_k - theta_x) and (beta*(y*y))*w_k)
 *   w_k = (w_k + dw) + sigma_eps*omega_k                 (the product kept as a product)
 *   w_k = w_k < -b ? -b : w_k;   w_k = w_k > b ? b : w_k (in this order; compare-and-select: a NaN stays a NaN, as in
 *                                                         the notebook's masked assignment)
 * omega is the stream of tnf_abc.h, a pure function of (seed, t, i, g, k): Philox4x32-10 with
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (g, t, i0 + i, k / 4)
 * and the block's four words -> normals 4b .. 4b + 3 by the Box-Muller of tnf_abc.h, bit for bit.  t is the caller's draw
 * index; when t_dev is non-NULL the kernel reads t from that device word (int64; its low 32 bits are the counter word)
 * instead, so that a captured step advances the stream by incrementing a device tensor.
 * Nothing depends on which lane, wave or launch evaluates a simulation.
 *
 * tnf_hebb_supported(n): 1 for 1 <= n <= TNF_HEBB_MAX_N, else 0.
 * tnf_hebb_launch_count(which): launches of the two kernels, a counter space of its own like tnf_abc_launch_count.
 * tnf_hebb_simulate_f32: z (N, 4), x (N_x, n), w0 (N_w0, n) with N_w0 in {1, N}, eps NULL (in-kernel stream) or
 *   (n_steps, N, n) standard normals (omega of step s, simulation i at eps[s, i]); out: w (N, n) the final state, traj
 *   NULL or (n_steps, N, n) the state after each step.  Limits: i0 >= 0, i0 + N <= 2^31, j0 >= 0, j0 + n_steps < 2^31,
 *   0 <= t < 2^31, N_x >= 1, sigma_eps >= 0.  Everything is checked before any launch: a NULL z / x / w0 / w, N_w0 not
 *   in {1, N}, a negative (or NaN) sigma_eps and the limits are TNF_EINVAL, n out of range is TNF_EUNSUPPORTED.
 *   N == 0 or n_steps == 0 return TNF_OK without a launch and without touching a buffer; with n_steps == 0 the result
 *   is the w0 rows, which the caller already has (hebb_ops.hebb_simulate returns them).
 * tnf_hebb_noise_f32: omega[c, a, k] = normal k of step j0 + c of simulation i0 + a in draw t, (n_j, n_i, n): exactly the
 *   normals the simulator consumes.  i0 + n_i <= 2^31, j0 + n_j < 2^31; an empty block returns TNF_OK without a launch.
 * The kernels use plain vector stores only: no atomics, no host synchronisation, no allocation. */
#ifndef TNF_HEBB_H
#define TNF_HEBB_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TNF_HEBB_MAX_N 64
enum { TNF_HEBB_COUNT_SIM = 0, TNF_HEBB_COUNT_NOISE = 1, TNF_HEBB_COUNTERS = 2 };
int tnf_hebb_supported(int32_t n);
int64_t tnf_hebb_launch_count(int32_t which);
int tnf_hebb_simulate_f32(const float* z, const float* x, const float* w0, const float* eps, float* w, float* traj,
                          const int64_t* t_dev, int64_t seed, int64_t t, int64_t i0, int64_t N, int64_t N_w0, int32_t n,
                          int32_t N_x, int64_t j0, int64_t n_steps, float sigma_eps, void* stream);
int tnf_hebb_noise_f32(float* omega, const int64_t* t_dev, int64_t seed, int64_t t, int64_t i0, int64_t n_i, int64_t j0,
                       int64_t n_j, int32_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_HEBB_H */
