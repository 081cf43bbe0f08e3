/* Mixture-of-Gaussians entries of libtnf_hip.so (density_estimator.py:57-237 of the reference).  Included by tnf.h;
 * a header of its own because the entries of tnf.h are a closed set whose host-side answers and marshalling are pinned
 * row by row (tests/cabi_host_table.json, tests/ops_marshalling.json).  Bound by torch_nf_amd/_lib.py MOG_SIGNATURES;
 * tests/test_mog_host.py keeps this header, the exports and that table in step.
 *
 * One parameter row has D_params = K (1 + D + D(D+1)/2) floats (:235-237): [logits (K) | mu_raw (K, D) | u (K, T)],
 * u the packed row-major upper triangle (torch.triu_indices order) of U_k, U_ii = exp(u_ii) (:114-129).
 * bounds: NULL, or [lb (D) | ub (D)] float32 on the device; then with m = (ub - lb)/2, c = (ub + lb)/2
 * mu = m tanh(mu_raw) + c, U_ii = exp(u_ii)/sqrt(m_i), Sigma_det = prod_i m_i exp(-2 u_ii) (:109-112, :124-134).
 * log_prob (:172-213), EPS = 1e-12, q_k = |U_k (z - mu_k)|^2:
 *   K == 1: lp = -(q + log(Sigma_det + EPS) + D log 2 pi)/2
 *   K  > 1: lp = log(sum_k alpha_k exp(-q_k/2) / sqrt((2 pi)^D Sigma_det_k + EPS) + EPS), alpha = softmax(logits)
 * evaluated in the log domain: the float64 value of that formula to float32 rounding at every D, its floor at
 * log EPS = -27.631 included.  float32 only.
 * z (M_z, N, D), params M_p rows of ld_params >= D_params floats, M_z and M_p in {1, M}; lp (M, N).
 *
 * tnf_mog_num_params: D_params, or -1 (D < 2, D > TNF_MOG_MAX_D, K < 1, or more than 2^30 - 1 floats).
 * tnf_mog_supported: 1 where the fused kernels exist: 2 <= D <= 16 and a prepared row (D_params + 2 K + 1 floats) within
 * 16 KB of LDS (K <= 26 at D = 16, K <= 178 at D = 5).  Every other shape runs a shape-generic kernel with run-time
 * loops, never a composition of other entries; TNF_OPT_FORCE_GENERIC selects it for a fused shape too.
 * tnf_mog_log_prob_backward_f32: from g_lp (M, N): g_params (M_p, D_params), contiguous, and, unless NULL, g_z
 * (M, N, D) -- per context even when M_z == 1 (the caller sums a broadcast z's gradient over the contexts).  g_params
 * is bit-reproducible: one launch, then at most one ordered sum over partial rows in the workspace; no float atomics.
 * tnf_mog_bwd_workspace_bytes: 0 for M_p == M with N < 64 (a lane owns a context's gradient row) and wherever one
 * workgroup owns a whole context; else M' G D_params 4 with G = min(ceil(N' / 128), max(1, 256 / M')) partial rows,
 * (M', N') = (1, M N) for M_p == 1 and (M, N) otherwise.  A workspace that is needed must be 16-byte aligned.
 * The generic backward (any D, any K) keeps every workgroup's arrays in the workspace instead of LDS: at most 512
 * workgroups walk the work, each with an area of its own behind the partial rows, and the query includes them.
 * tnf_mog_sample_f32 (:145-170): params M rows; u (M, N) uniform, e1, e2 (M, N, D) standard normal;
 * k = #{j : cumsum(alpha)_j <= u}, at most K - 1; z = mu_k + U_k^-1 e1 + sqrt(0.001) e2 ~ N(mu_k, Sigma_k + 0.001 I)
 * (:152); the same launch writes log_q = tnf_mog_log_prob_f32(z, params), bit for bit.
 * tnf_mog_launch_count: launches of the FUSED kernels, a counter space of its own like tnf_ef_launch_count. */
#ifndef TNF_MOG_H
#define TNF_MOG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TNF_MOG_MAX_D 4096
enum { TNF_MOG_COUNT_LOGPROB = 0, TNF_MOG_COUNT_LOGPROB_BWD = 1, TNF_MOG_COUNT_SAMPLE = 2, TNF_MOG_COUNTERS = 3 };
int64_t tnf_mog_num_params(int32_t D, int32_t K);
int tnf_mog_supported(int32_t D, int32_t K);
int64_t tnf_mog_launch_count(int32_t which);
int tnf_mog_log_prob_f32(const float* z, const float* params, const float* bounds, float* lp, int64_t M_z, int64_t M_p,
                         int64_t N, int32_t D, int32_t K, int64_t ld_params, void* stream);
int64_t tnf_mog_bwd_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t K);
int tnf_mog_log_prob_backward_f32(const float* z, const float* params, const float* bounds, const float* g_lp, float* g_z,
                                  float* g_params, int64_t M_z, int64_t M_p, int64_t N, int32_t D, int32_t K,
                                  int64_t ld_params, void* workspace, int64_t workspace_bytes, void* stream);
int tnf_mog_sample_f32(const float* params, const float* bounds, const float* u, const float* e1, const float* e2, float* z,
                       float* log_q, int64_t M, int64_t N, int32_t D, int32_t K, int64_t ld_params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_MOG_H */
