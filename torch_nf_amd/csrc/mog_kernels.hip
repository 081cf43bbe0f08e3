// Mixture of Gaussians (density_estimator.py:57-237 of the reference): log_prob, its backward and sampling.
// One parameter row is [logits (K) | mu_raw (K*D) | u (K*T)], T = D(D+1)/2, u the packed row-major upper triangle of
// the factor U_k (U_ii = exp(u_ii), with bounds / sqrt(m_i)); Sigma_inv_k = U_k^T U_k is never formed:
//   q_k = |U_k (z - mu_k)|^2,  y_i = sum_{j >= i} U_ij d_j          T + D FMAs per component, nothing below the diagonal
//   K == 1   lp = -(q + log(Sigma_det + EPS) + D log 2 pi) / 2
//   K  > 1   lp = log(sum_k alpha_k exp(-q_k / 2) / sqrt((2 pi)^D Sigma_det_k + EPS) + EPS),  EPS = 1e-12
// evaluated in the log domain ((2 pi)^D overflows float32 from D = 48): with L_k = D log 2 pi + log Sigma_det_k,
//   a_k = log alpha_k - logaddexp(L_k, log EPS) / 2 - q_k / 2,   lp = logsumexp(a_1 .. a_K, log EPS)
// which is the reference's formula, EPS terms and the floor at log EPS included.
// A PREPARED row holds what depends on the row alone, computed once per staged row (mog_stage_rows):
//   [c_k - C (K) | mu (K*D), bounded | U (K*T), diagonal exponentiated and scaled | log alpha_k (K) | rho_k (K) | C]
//   c_k = a_k + q_k / 2, C = max_k c_k;  rho_k = exp(L_k) / (exp(L_k) + EPS), the derivative of the normaliser's EPS
//   term.  The kernels work with a_k - C and add C to lp last: C carries the -D/2 log 2 pi every component shares, and
//   without it a_k - lp, the log of a responsibility, would be rounded at the magnitude of lp instead of its own.
// Two layouts, both with one sample per lane:
//   shared row   (M_p == 1, or N >= 64 per context): a workgroup = one context x a run of 128-sample tiles; its
//                prepared row sits in LDS and is read at wave-uniform addresses (broadcast), z is staged through LDS
//                at an odd row stride so that every global access is coalesced.
//   row per lane (M_p == M and N < 64): a workgroup stages the rows of a run of contexts through LDS in one coalesced
//                sweep -- each row leaves HBM exactly once -- prepares them in place, and every lane reads its row at
//                an odd stride (conflict-free).
// Fused kernels: D a template parameter, 2 <= D <= 16, vectors in registers, K a run-time loop.  The generic forward
// kernel reads raw rows from global memory with run-time loops (any D, any K); the generic backward is the fused
// backward's code (D = 0 instantiation) with every workgroup's arrays in an area of the workspace instead of LDS, so it
// too serves any D and any K.
// Backward: g_params is reduced in a fixed order and is bit-reproducible.  Row per lane: a lane owns a context, walks
// its N < 64 samples in order and owns its gradient row in LDS, which leaves coalesced -- no reduction.  Shared row:
// every workgroup owns one partial row; each entry of it is owned by one thread, which adds the tile's samples in
// sample order; an ordered pass adds the partial rows (the mechanism of ef_geta_partial_kernel).  No float atomics.
#include "launch.h"

namespace tnf {

#define MOG_LN_EPS (-27.631021115928547f)
#define MOG_LOG_2PI 1.8378770664093453f
#define MOG_SQRT_JITTER 0.03162277660168379f  // sqrt(0.001): the reference samples N(mu, Sigma + 0.001 I) (:152)
enum { MOG_TILE = 128, MOG_LDS_FLOATS = 15360, MOG_ROW_MAX = 4096, MOG_MIN_SHARED_N = 64 };

__host__ __device__ __forceinline__ int mog_tri_off(int i, int D) { return i * D - i * (i - 1) / 2; }
__host__ __device__ __forceinline__ int64_t mog_P(int D, int K) { return (int64_t)K * (1 + D + (int64_t)D * (D + 1) / 2); }
__host__ __device__ __forceinline__ int mog_ldp(int D, int K) { return (int)((mog_P(D, K) + 2 * K + 1) | 1); }

__device__ __forceinline__ float mog_logaddexp(float a, float b) {
    const float hi = fmaxf(a, b), lo = fminf(a, b);
    return hi + log1pf(expf(lo - hi));
}
__device__ __forceinline__ float mog_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// Stage `rc` raw rows into LDS (row stride LDP, odd) in one coalesced sweep and prepare them in place.
// bnd: [m (D) | c (D)] of the bounds, filled here when bounds != NULL.  Ends with a barrier.
__device__ void mog_stage_rows(float* rows, float* bnd, const float* __restrict__ params, int64_t ld, int rc, int D, int K,
                               int P, int LDP, const float* __restrict__ bounds, int tid) {
    const int T = D * (D + 1) / 2;
    for (int idx = tid; idx < rc * P; idx += MOG_TILE) {
        const int r = idx / P, j = idx - r * P;
        rows[r * LDP + j] = params[(int64_t)r * ld + j];
    }
    if (bounds)
        for (int d = tid; d < D; d += MOG_TILE) {
            const float lb = bounds[d], ub = bounds[D + d];
            bnd[d] = 0.5f * (ub - lb);
            bnd[D + d] = 0.5f * (ub + lb);
        }
    __syncthreads();
    for (int r = tid; r < rc; r += MOG_TILE) {  // the per-component constants: one thread per row
        float* row = rows + r * LDP;
        float ldm = 0.0f;
        if (bounds)
            for (int d = 0; d < D; ++d) ldm += logf(bnd[d]);
        float mx = row[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, row[k]);
        float s = 0.0f;
        for (int k = 0; k < K; ++k) s += expf(row[k] - mx);
        const float lse = mx + logf(s);
        for (int k = 0; k < K; ++k) {
            const float* u = row + K + K * D + k * T;
            float sd = 0.0f;
            for (int i = 0; i < D; ++i) sd += u[mog_tri_off(i, D)];
            const float Ls = fmaf(-2.0f, sd, ldm);  // log Sigma_det
            if (K == 1) {
                row[P] = 0.0f;
                row[P + 1] = mog_sigmoid(Ls - MOG_LN_EPS);
                row[P + 2] = 0.0f;
                row[0] = -0.5f * (mog_logaddexp(Ls, MOG_LN_EPS) + (float)D * MOG_LOG_2PI);
            } else {
                const float L = Ls + (float)D * MOG_LOG_2PI, la = row[k] - lse;
                row[P + k] = la;
                row[P + K + k] = mog_sigmoid(L - MOG_LN_EPS);
                row[k] = fmaf(-0.5f, mog_logaddexp(L, MOG_LN_EPS), la);
            }
        }
        if (K > 1) {
            float C = row[0];
            for (int k = 1; k < K; ++k) C = fmaxf(C, row[k]);
            for (int k = 0; k < K; ++k) row[k] -= C;
            row[P + 2 * K] = C;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < rc * K * D; idx += MOG_TILE) {  // bounded means, the factor's diagonal
        const int r = idx / (K * D), rem = idx - r * (K * D), k = rem / D, i = rem - k * D;
        float* row = rows + r * LDP;
        float* ud = row + K + K * D + k * T + mog_tri_off(i, D);
        const float e = expf(*ud);
        if (bounds) {
            float* mu = row + K + k * D + i;
            *mu = fmaf(bnd[i], tanhf(*mu), bnd[D + i]);
            *ud = e / sqrtf(bnd[i]);
        } else {
            *ud = e;
        }
    }
    __syncthreads();
}

// d = z - mu_k, y = U_k d for component k of a prepared row; returns a_k.  DT > 0: D = DT, every loop unrolls and the
// vectors are registers; DT == 0: run-time D, the vectors are where the caller put them.
template <int DT>
__device__ __forceinline__ float mog_component(const float* row, int k, int K, int Drt, const float* z, float* d, float* y) {
    const int D = DT ? DT : Drt;
    const int T = D * (D + 1) / 2;
    const float* mu = row + K + k * D;
    const float* U = row + K + K * D + k * T;
#pragma unroll DT ? 16 : 1
    for (int i = 0; i < D; ++i) d[i] = z[i] - mu[i];
    float q = 0.0f;
#pragma unroll DT ? 16 : 1
    for (int i = 0; i < D; ++i) {
        const int base = i * D - i * (i - 1) / 2 - i;  // U[i][j] = U[base + j]
        float acc = 0.0f;
#pragma unroll DT ? 16 : 1
        for (int j = i; j < D; ++j) acc = fmaf(U[base + j], d[j], acc);
        y[i] = acc;
        q = fmaf(acc, acc, q);
    }
    return fmaf(-0.5f, q, row[k]);
}

// lp - C (C = row[P + 2K], 0 for K == 1)
template <int DT>
__device__ __forceinline__ float mog_lp(const float* row, int K, int Drt, const float* z, float* d, float* y) {
    if (K == 1) return mog_component<DT>(row, 0, 1, Drt, z, d, y);
    const int D = DT ? DT : Drt;
    float m = MOG_LN_EPS - row[K * (1 + D + D * (D + 1) / 2) + 2 * K], s = 1.0f;  // the EPS term opens the log-sum-exp
    for (int k = 0; k < K; ++k) {
        const float a = mog_component<DT>(row, k, K, Drt, z, d, y);
        if (a > m) {
            s = fmaf(s, expf(m - a), 1.0f);
            m = a;
        } else {
            s += expf(a - m);
        }
    }
    return m + logf(s);
}

// the sampling map: component k = #{j : cumsum(alpha)_j <= u} (at most K - 1), z = mu_k + U_k^-1 e1 + sqrt(0.001) e2
struct MogDraws {
    const float* u;   // (M, N)
    const float* e1;  // (M, N, D)
    const float* e2;  // (M, N, D)
    float* z;         // (M, N, D) out
};

template <int DT>
__device__ __forceinline__ void mog_draw(const float* row, int K, int P, float u, const float* __restrict__ e1,
                                         const float* __restrict__ e2, float* z) {
    constexpr int T = DT * (DT + 1) / 2;
    int k = 0;
    if (K > 1) {
        float c = 0.0f;
        for (int j = 0; j < K; ++j) {
            c += expf(row[P + j]);
            k += c <= u ? 1 : 0;
        }
        if (k > K - 1) k = K - 1;
    }
    const float* mu = row + K + k * DT;
    const float* U = row + K + K * DT + k * T;
    float x[DT];
#pragma unroll DT ? 16 : 1
    for (int i = DT - 1; i >= 0; --i) {
        const int base = i * DT - i * (i - 1) / 2 - i;
        float acc = e1[i];
#pragma unroll DT ? 16 : 1
        for (int j = i + 1; j < DT; ++j) acc = fmaf(-U[base + j], x[j], acc);
        x[i] = acc / U[base + i];
    }
#pragma unroll DT ? 16 : 1
    for (int i = 0; i < DT; ++i) z[i] = fmaf(MOG_SQRT_JITTER, e2[i], mu[i] + x[i]);
}

// ---------------------------------------------------------------------------
// log_prob (and sampling + log_q), fused, shared row
// ---------------------------------------------------------------------------
template <int DT, bool SAMPLE>
__global__ void __launch_bounds__(MOG_TILE)
mog_lp_shared_kernel(const float* __restrict__ z, const float* __restrict__ params, const float* __restrict__ bounds,
                     float* __restrict__ lp, int64_t Mz, int64_t Mp, int64_t M, int64_t N, int K, int64_t ld,
                     int tiles_per_wg, MogDraws dr) {
    extern __shared__ __attribute__((aligned(16))) float mog_smem[];
    constexpr int LD = DT | 1;
    const int P = (int)mog_P(DT, K), LDP = mog_ldp(DT, K);
    float* row = mog_smem;
    float* bnd = row + LDP;
    float* tile = bnd + 2 * DT;
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    mog_stage_rows(row, bnd, params + (Mp == 1 ? 0 : m) * ld, ld, 1, DT, K, P, LDP, bounds, tid);
    const float* zm = z + (Mz == 1 ? 0 : m) * N * DT;
    for (int t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * MOG_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)MOG_TILE ? (N - n0) : (int64_t)MOG_TILE);
        float zr[DT], d[DT], y[DT];
        if (SAMPLE) {
            if (tid < nr) {
                const int64_t s = m * N + n0 + tid;
                mog_draw<DT>(row, K, P, dr.u[s], dr.e1 + s * DT, dr.e2 + s * DT, zr);
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < DT; ++i) dr.z[s * DT + i] = zr[i];
            }
        } else {
            __syncthreads();
            const float* src = zm + n0 * DT;
            for (int idx = tid; idx < nr * DT; idx += MOG_TILE) {
                const int r = idx / DT, c = idx - r * DT;
                tile[r * LD + c] = src[idx];
            }
            __syncthreads();
            if (tid < nr) {
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < DT; ++i) zr[i] = tile[tid * LD + i];
            }
        }
        if (tid < nr) lp[m * N + n0 + tid] = mog_lp<DT>(row, K, DT, zr, d, y) + row[P + 2 * K];
    }
}

// ---------------------------------------------------------------------------
// log_prob (and sampling + log_q), fused, row per lane: workgroup = contexts [m0, m0 + rc)
// ---------------------------------------------------------------------------
template <int DT, bool SAMPLE>
__global__ void __launch_bounds__(MOG_TILE)
mog_lp_lane_kernel(const float* __restrict__ z, const float* __restrict__ params, const float* __restrict__ bounds,
                   float* __restrict__ lp, int64_t Mz, int64_t M, int64_t N, int K, int64_t ld, int rc, MogDraws dr) {
    extern __shared__ __attribute__((aligned(16))) float mog_smem[];
    const int P = (int)mog_P(DT, K), LDP = mog_ldp(DT, K);
    float* rows = mog_smem;
    float* bnd = rows + rc * LDP;
    const int64_t m0 = (int64_t)blockIdx.x * rc;
    const int nr = (int)((M - m0) < (int64_t)rc ? (M - m0) : (int64_t)rc);
    const int tid = threadIdx.x;
    mog_stage_rows(rows, bnd, params + m0 * ld, ld, nr, DT, K, P, LDP, bounds, tid);
    const int items = nr * (int)N;
    for (int it = tid; it < items; it += MOG_TILE) {
        const int r = it / (int)N, n = it - r * (int)N;
        const int64_t m = m0 + r;
        const float* row = rows + r * LDP;
        float zr[DT], d[DT], y[DT];
        if (SAMPLE) {
            const int64_t s = m * N + n;
            mog_draw<DT>(row, K, P, dr.u[s], dr.e1 + s * DT, dr.e2 + s * DT, zr);
#pragma unroll DT ? 16 : 1
            for (int i = 0; i < DT; ++i) dr.z[s * DT + i] = zr[i];
        } else {
            const float* src = z + ((Mz == 1 ? 0 : m) * N + n) * DT;
#pragma unroll DT ? 16 : 1
            for (int i = 0; i < DT; ++i) zr[i] = src[i];
        }
        lp[m * N + n] = mog_lp<DT>(row, K, DT, zr, d, y) + row[P + 2 * K];
    }
}

// ---------------------------------------------------------------------------
// log_prob (and sampling + log_q), shape-generic: one sample per lane, raw rows from global memory, run-time loops
// ---------------------------------------------------------------------------
template <bool SAMPLE>
__global__ void __launch_bounds__(256)
mog_lp_generic_kernel(const float* __restrict__ z, const float* __restrict__ params, const float* __restrict__ bounds,
                      float* __restrict__ lp, int64_t Mz, int64_t Mp, int64_t M, int64_t N, int D, int K, int64_t ld,
                      MogDraws dr) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * N) return;
    const int64_t m = idx / N, n = idx - m * N;
    const int T = D * (D + 1) / 2;
    const float* p = params + (Mp == 1 ? 0 : m) * ld;
    const float* mur = p + K;
    const float* ur = p + K + (int64_t)K * D;
    float ldm = 0.0f;
    if (bounds)
        for (int i = 0; i < D; ++i) ldm += logf(0.5f * (bounds[D + i] - bounds[i]));
    float mx = p[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, p[k]);
    float se = 0.0f;
    for (int k = 0; k < K; ++k) se += expf(p[k] - mx);
    const float lse = mx + logf(se);
    const float* zr = SAMPLE ? nullptr : z + ((Mz == 1 ? 0 : m) * N + n) * D;
    if (SAMPLE) {
        int k = 0;
        if (K > 1) {
            const float u = dr.u[idx];
            float c = 0.0f;
            for (int j = 0; j < K; ++j) {
                c += expf(p[j] - lse);
                k += c <= u ? 1 : 0;
            }
            if (k > K - 1) k = K - 1;
        }
        float* x = dr.z + idx * D;  // the lane's own output row holds the back-substitution
        const float* e1 = dr.e1 + idx * D;
        const float* e2 = dr.e2 + idx * D;
        const float* u_k = ur + (int64_t)k * T;
        for (int i = D - 1; i >= 0; --i) {
            const int base = mog_tri_off(i, D) - i;
            float acc = e1[i];
            for (int j = i + 1; j < D; ++j) acc = fmaf(-u_k[base + j], x[j], acc);
            float uii = expf(u_k[base + i]);
            if (bounds) uii = uii / sqrtf(0.5f * (bounds[D + i] - bounds[i]));
            x[i] = acc / uii;
        }
        for (int i = 0; i < D; ++i) {
            float mu = mur[k * D + i];
            if (bounds) mu = fmaf(0.5f * (bounds[D + i] - bounds[i]), tanhf(mu), 0.5f * (bounds[D + i] + bounds[i]));
            x[i] = fmaf(MOG_SQRT_JITTER, e2[i], mu + x[i]);
        }
        zr = x;
    }
    float rm = MOG_LN_EPS, rs = 1.0f, a = 0.0f;
    for (int k = 0; k < K; ++k) {
        const float* u_k = ur + (int64_t)k * T;
        float sd = 0.0f, q = 0.0f;
        for (int i = 0; i < D; ++i) {
            const int base = mog_tri_off(i, D) - i;
            sd += u_k[base + i];
            float acc = 0.0f;
            for (int j = i; j < D; ++j) {
                float mu = mur[k * D + j], uij = u_k[base + j];
                if (bounds) mu = fmaf(0.5f * (bounds[D + j] - bounds[j]), tanhf(mu), 0.5f * (bounds[D + j] + bounds[j]));
                if (j == i) {
                    uij = expf(uij);
                    if (bounds) uij = uij / sqrtf(0.5f * (bounds[D + i] - bounds[i]));
                }
                acc = fmaf(uij, zr[j] - mu, acc);
            }
            q = fmaf(acc, acc, q);
        }
        const float Ls = fmaf(-2.0f, sd, ldm);
        if (K == 1) {
            a = fmaf(-0.5f, q, -0.5f * (mog_logaddexp(Ls, MOG_LN_EPS) + (float)D * MOG_LOG_2PI));
        } else {
            const float c = fmaf(-0.5f, mog_logaddexp(Ls + (float)D * MOG_LOG_2PI, MOG_LN_EPS), p[k] - lse);
            a = fmaf(-0.5f, q, c);
            if (a > rm) {
                rs = fmaf(rs, expf(rm - a), 1.0f);
                rm = a;
            } else {
                rs += expf(a - rm);
            }
        }
    }
    lp[idx] = K == 1 ? a : rm + logf(rs);
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// the tanh chain of the bounded means, applied when a gradient row leaves LDS: raw mu from global memory
__device__ __forceinline__ float mog_mu_chain(float v, int j, int D, int K, const float* bnd, const float* __restrict__ praw) {
    if (j < K || j >= K + K * D) return v;
    const int i = (j - K) % D;
    const float t = tanhf(praw[j]);
    return v * bnd[i] * (1.0f - t * t);
}

// Row per lane: a lane owns context m0 + tid, its N samples in order and gradient row `gr` in LDS.
template <int DT>
__global__ void __launch_bounds__(MOG_TILE)
mog_bwd_lane_kernel(const float* __restrict__ z, const float* __restrict__ params, const float* __restrict__ bounds,
                    const float* __restrict__ g_lp, float* __restrict__ g_z, float* __restrict__ g_params, int64_t Mz,
                    int64_t M, int64_t N, int Drt, int K, int64_t ld, int rc, float* gws, int64_t area) {
    extern __shared__ __attribute__((aligned(16))) float mog_smem[];
    const int D = DT ? DT : Drt;
    const int T = D * (D + 1) / 2, P = (int)mog_P(D, K), LDP = mog_ldp(D, K), LS = (3 * D) | 1;
    // DT > 0: the workgroup's arrays are LDS; DT == 0 (any D, any K): its own area of the workspace, same code
    float* rows = DT ? mog_smem : gws + (int64_t)blockIdx.x * area;
    float* grows = rows + rc * LDP;
    float* bnd = grows + rc * LDP;
    float* scratch = bnd + 2 * D;  // DT == 0 only: [d | y | g_z] per lane
    const int tid = threadIdx.x;
    const int64_t nchunks = (M + rc - 1) / rc;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t m0 = ch * rc;
    const int nr = (int)((M - m0) < (int64_t)rc ? (M - m0) : (int64_t)rc);
    for (int idx = tid; idx < nr * LDP; idx += MOG_TILE) grows[idx] = 0.0f;
    mog_stage_rows(rows, bnd, params + m0 * ld, ld, nr, D, K, P, LDP, bounds, tid);
    if (tid < nr) {
        const int64_t m = m0 + tid;
        const float* row = rows + tid * LDP;
        float* gr = grows + tid * LDP;
        float zl[DT ? DT : 1], dl[DT ? DT : 1], yl[DT ? DT : 1], gl[DT ? DT : 1];
        float* d = DT ? dl : scratch + tid * LS;
        float* y = DT ? yl : scratch + tid * LS + D;
        float* gz = DT ? gl : scratch + tid * LS + 2 * D;
        for (int64_t n = 0; n < N; ++n) {
            const float* src = z + ((Mz == 1 ? 0 : m) * N + n) * D;
            const float* zr = src;
            if (DT) {
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) zl[i] = src[i];
                zr = zl;
            }
            const float g = g_lp[m * N + n];
            const float lp = K == 1 ? 0.0f : mog_lp<DT>(row, K, D, zr, d, y);
#pragma unroll DT ? 16 : 1
            for (int i = 0; i < D; ++i) gz[i] = 0.0f;
            float R = 0.0f;
            for (int k = 0; k < K; ++k) {
                const float a = mog_component<DT>(row, k, K, D, zr, d, y);
                const float r = K == 1 ? g : g * expf(a - lp);
                const float* U = row + K + K * D + k * T;
                float* gU = gr + K + K * D + k * T;
                const float rho = row[P + K + k];
                R += r;
                gr[k] += r;
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) y[i] *= r;
#pragma unroll DT ? 16 : 1
                for (int j = 0; j < D; ++j) {  // (U^T y)_j
                    float v = 0.0f;
#pragma unroll DT ? 16 : 1
                    for (int i = 0; i <= j; ++i) v = fmaf(U[i * D - i * (i - 1) / 2 - i + j], y[i], v);
                    gr[K + k * D + j] += v;
                    gz[j] -= v;
                }
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) {
                    const int base = i * D - i * (i - 1) / 2 - i;
                    gU[base + i] += fmaf(-U[base + i], y[i] * d[i], rho * r);
#pragma unroll DT ? 16 : 1
                    for (int j = i + 1; j < D; ++j) gU[base + j] -= y[i] * d[j];
                }
            }
            if (K > 1)
                for (int k = 0; k < K; ++k) gr[k] -= expf(row[P + k]) * R;
            if (g_z) {
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) g_z[(m * N + n) * D + i] = gz[i];
            }
        }
        if (K == 1) gr[0] = 0.0f;  // alpha is ignored
    }
    __syncthreads();
    for (int idx = tid; idx < nr * P; idx += MOG_TILE) {
        const int r = idx / P, j = idx - r * P;
        float v = grows[r * LDP + j];
        if (bounds) v = mog_mu_chain(v, j, D, K, bnd, params + (m0 + r) * ld);
        g_params[(m0 + r) * P + j] = v;
    }
    __syncthreads();  // the next chunk restages
    }
}

// Shared row: workgroup (chunk c, context m) walks its tiles in order and owns partial row (m, c); per component the
// lanes stage [r y (D) | d (D) | r | R] of their samples in LDS and thread e owns entry e of the component's gradient.
template <int DT>
__global__ void __launch_bounds__(MOG_TILE)
mog_bwd_shared_kernel(const float* __restrict__ z, const float* __restrict__ params, const float* __restrict__ bounds,
                      const float* __restrict__ g_lp, float* __restrict__ g_z, float* __restrict__ partial, int64_t Mz,
                      int64_t Mp, int64_t M, int64_t N, int Drt, int K, int64_t ld, int G, int64_t tiles_per_chunk,
                      float* gws, int64_t area) {
    extern __shared__ __attribute__((aligned(16))) float mog_smem[];
    const int D = DT ? DT : Drt;
    const int T = D * (D + 1) / 2, P = (int)mog_P(D, K), LDP = mog_ldp(D, K), LS = (3 * D + 2) | 1, E = 1 + D + T;
    // DT > 0: the workgroup's arrays are LDS; DT == 0 (any D, any K): its own area of the workspace, same code
    float* row = DT ? mog_smem : gws + (int64_t)blockIdx.x * area;
    float* part = row + LDP;
    float* bnd = part + P;
    float* S = bnd + 2 * D;
    const int tid = threadIdx.x;
    for (int64_t w = blockIdx.x; w < M * G; w += gridDim.x) {  // work item = (context m, chunk c)
    const int64_t m = w / G;
    const int c = (int)(w - m * G);
    const float* praw = params + (Mp == 1 ? 0 : m) * ld;
    for (int j = tid; j < P; j += MOG_TILE) part[j] = 0.0f;
    mog_stage_rows(row, bnd, praw, ld, 1, D, K, P, LDP, bounds, tid);
    float* Sl = S + tid * LS;
    float zl[DT ? DT : 1], dl[DT ? DT : 1], yl[DT ? DT : 1], gl[DT ? DT : 1];
    float* d = DT ? dl : Sl + D;
    float* y = DT ? yl : Sl;
    float* gz = DT ? gl : Sl + 2 * D + 2;
    const int64_t ntiles = (N + MOG_TILE - 1) / MOG_TILE;
    const int64_t t0 = (int64_t)c * tiles_per_chunk;
    int64_t t1 = t0 + tiles_per_chunk;
    if (t1 > ntiles) t1 = ntiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t n0 = t * MOG_TILE;
        const int nr = (int)((N - n0) < (int64_t)MOG_TILE ? (N - n0) : (int64_t)MOG_TILE);
        const bool active = tid < nr;
        const int64_t n = n0 + tid;
        const float* zr = z;
        float g = 0.0f, lp = 0.0f, R = 0.0f;
        if (active) {
            const float* src = z + ((Mz == 1 ? 0 : m) * N + n) * D;
            zr = src;
            if (DT) {
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) zl[i] = src[i];
                zr = zl;
            }
            g = g_lp[m * N + n];
        }
        __syncthreads();  // the previous tile's readers of S are done (DT == 0: d, y live there)
        if (active) {
            if (K > 1) lp = mog_lp<DT>(row, K, D, zr, d, y);
#pragma unroll DT ? 16 : 1
            for (int i = 0; i < D; ++i) gz[i] = 0.0f;
        }
        for (int k = 0; k < K; ++k) {
            const float* U = row + K + K * D + k * T;
            if (k > 0) __syncthreads();
            if (active) {
                const float a = mog_component<DT>(row, k, K, D, zr, d, y);
                const float r = K == 1 ? g : g * expf(a - lp);
                R += r;
#pragma unroll DT ? 16 : 1
                for (int i = 0; i < D; ++i) {
                    y[i] *= r;
                    Sl[i] = y[i];
                    Sl[D + i] = d[i];
                }
                Sl[2 * D] = r;
#pragma unroll DT ? 16 : 1
                for (int j = 0; j < D; ++j) {
                    float v = 0.0f;
#pragma unroll DT ? 16 : 1
                    for (int i = 0; i <= j; ++i) v = fmaf(U[i * D - i * (i - 1) / 2 - i + j], y[i], v);
                    gz[j] -= v;
                }
            }
            __syncthreads();
            for (int e = tid; e < E; e += MOG_TILE) {
                if (e == 0) {
                    if (K > 1) {
                        float acc = 0.0f;
                        for (int s = 0; s < nr; ++s) acc += S[s * LS + 2 * D];
                        part[k] += acc;
                    }
                } else if (e <= D) {
                    const int j = e - 1;
                    float acc = 0.0f;
                    for (int s = 0; s < nr; ++s) {
                        float v = 0.0f;
                        for (int i = 0; i <= j; ++i) v = fmaf(U[mog_tri_off(i, D) - i + j], S[s * LS + i], v);
                        acc += v;
                    }
                    part[K + k * D + j] += acc;
                } else {
                    int p = e - 1 - D, i = 0;
                    while (p >= D - i) {
                        p -= D - i;
                        ++i;
                    }
                    const int j = i + p;
                    float acc = 0.0f, rs = 0.0f;
                    for (int s = 0; s < nr; ++s) {
                        acc = fmaf(S[s * LS + i], S[s * LS + D + j], acc);
                        rs += S[s * LS + 2 * D];
                    }
                    part[K + K * D + k * T + (e - 1 - D)] += i == j ? fmaf(-U[e - 1 - D], acc, row[P + K + k] * rs) : -acc;
                }
            }
        }
        if (K > 1) {
            __syncthreads();
            if (active) Sl[2 * D + 1] = R;
            __syncthreads();
            for (int k = tid; k < K; k += MOG_TILE) {
                float acc = 0.0f;
                for (int s = 0; s < nr; ++s) acc += S[s * LS + 2 * D + 1];
                part[k] -= expf(row[P + k]) * acc;
            }
        }
        if (g_z && active) {
#pragma unroll DT ? 16 : 1
            for (int i = 0; i < D; ++i) g_z[(m * N + n) * D + i] = gz[i];
        }
    }
    __syncthreads();
    float* out = partial + (m * G + c) * (int64_t)P;
    for (int j = tid; j < P; j += MOG_TILE) {
        float v = part[j];
        if (bounds) v = mog_mu_chain(v, j, D, K, bnd, praw);
        out[j] = v;
    }
    __syncthreads();  // the next work item restages
    }
}

// g_params[mp][j] = sum over the G partial rows of context mp, in row order
__global__ void __launch_bounds__(256)
mog_reduce_kernel(const float* __restrict__ partial, float* __restrict__ g_params, int64_t rows, int P, int G) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * P) return;
    const int64_t mp = idx / P;
    const int j = (int)(idx - mp * P);
    float acc = 0.0f;
    for (int c = 0; c < G; ++c) acc += partial[(mp * G + c) * (int64_t)P + j];
    g_params[idx] = acc;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t mog_num_params(int D, int K) {
    if (D < 2 || K < 1 || D > TNF_MOG_MAX_D) return -1;
    const int64_t P = mog_P(D, K);
    return P > 0x3fffffff ? -1 : P;
}

bool mog_fused_supported(int D, int K) {
    return D >= 2 && D <= 16 && K >= 1 && mog_P(D, K) + 2 * (int64_t)K + 2 <= MOG_ROW_MAX;
}

// a call's geometry: a shared row makes the (M, N) split meaningless, so M_p == 1 runs as one context of M * N samples
struct MogGeom {
    bool shared;
    int64_t M, N, Mz, Mp;
};
static MogGeom mog_geom(int64_t Mz, int64_t Mp, int64_t N) {
    MogGeom g;
    const int64_t M = Mz > Mp ? Mz : Mp;
    if (Mp == 1) {
        g.shared = true;
        g.M = 1, g.N = M * N, g.Mz = 1, g.Mp = 1;
    } else {
        g.shared = N >= MOG_MIN_SHARED_N;
        g.M = M, g.N = N, g.Mz = Mz, g.Mp = Mp;
    }
    return g;
}

static int mog_tiles_per_wg(int64_t M, int64_t N, int64_t* bx) {
    const int64_t tiles = (N + MOG_TILE - 1) / MOG_TILE;
    int64_t want = 2048 / (M < 2048 ? M : 2048);  // workgroups per context: the device eight times over
    if (want < 1) want = 1;
    int64_t per = (tiles + want - 1) / want;
    if (per < 1) per = 1;
    if (per > 64) per = 64;
    *bx = (tiles + per - 1) / per;
    return (int)per;
}

static int mog_lane_rows(int D, int K, int copies, int extra) {  // contexts per workgroup of a row-per-lane kernel
    int64_t rc = ((int64_t)MOG_LDS_FLOATS - 2 * D - extra) / ((int64_t)copies * mog_ldp(D, K));
    if (rc > MOG_TILE) rc = MOG_TILE;
    return rc < 1 ? 0 : (int)rc;
}

#define MOG_CASE(Dv, KERNEL, ...)                                                          \
    case Dv:                                                                               \
        if (launch_lds(what, KERNEL<Dv, SAMPLE>, grid, dim3(MOG_TILE), smem, st, __VA_ARGS__)) return TNF_ELAUNCH; \
        break;
#define MOG_SWITCH(KERNEL, ...)                                                                                      \
    switch (D) {                                                                                                     \
        MOG_CASE(2, KERNEL, __VA_ARGS__) MOG_CASE(3, KERNEL, __VA_ARGS__) MOG_CASE(4, KERNEL, __VA_ARGS__)           \
        MOG_CASE(5, KERNEL, __VA_ARGS__) MOG_CASE(6, KERNEL, __VA_ARGS__) MOG_CASE(7, KERNEL, __VA_ARGS__)           \
        MOG_CASE(8, KERNEL, __VA_ARGS__) MOG_CASE(9, KERNEL, __VA_ARGS__) MOG_CASE(10, KERNEL, __VA_ARGS__)          \
        MOG_CASE(11, KERNEL, __VA_ARGS__) MOG_CASE(12, KERNEL, __VA_ARGS__) MOG_CASE(13, KERNEL, __VA_ARGS__)        \
        MOG_CASE(14, KERNEL, __VA_ARGS__) MOG_CASE(15, KERNEL, __VA_ARGS__) MOG_CASE(16, KERNEL, __VA_ARGS__)        \
        default:                                                                                                     \
            return fail(TNF_EUNSUPPORTED, "mog: no fused kernel for D=%d", D);                                       \
    }

// log_prob of z, or (dr != NULL) draw z = dr->z first and evaluate it: one launch either way
template <bool SAMPLE>
static int mog_launch_forward(const float* z, const float* params, const float* bounds, float* lp, int64_t Mz0, int64_t Mp0,
                              int64_t N0, int D, int K, int64_t ld, const MogDraws& dr, hipStream_t st) {
    const char* what = SAMPLE ? "mog_sample" : "mog_log_prob";
    const MogGeom g = mog_geom(Mz0, Mp0, N0);
    if (g.M == 0 || g.N == 0) return TNF_OK;
    if (!g_force_generic && mog_fused_supported(D, K)) {
        const int LDP = mog_ldp(D, K);
        if (g.shared) {
            int64_t bx;
            const int per = mog_tiles_per_wg(g.M, g.N, &bx);
            const dim3 grid = grid_xm(bx, g.M);
            const size_t smem = ((size_t)LDP + 2 * D + (size_t)MOG_TILE * (D | 1)) * sizeof(float);
            MOG_SWITCH(mog_lp_shared_kernel, z, params, bounds, lp, g.Mz, g.Mp, g.M, g.N, K, ld, per, dr)
        } else {
            const int rc = mog_lane_rows(D, K, 1, 0);
            const int64_t blocks = (g.M + rc - 1) / rc;
            if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", what);
            const dim3 grid((unsigned)blocks);
            const size_t smem = ((size_t)rc * LDP + 2 * D) * sizeof(float);
            MOG_SWITCH(mog_lp_lane_kernel, z, params, bounds, lp, g.Mz, g.M, g.N, K, ld, rc, dr)
        }
        mog_count(SAMPLE ? TNF_MOG_COUNT_SAMPLE : TNF_MOG_COUNT_LOGPROB);
        return check_launch(what);
    }
    const int64_t blocks = (g.M * g.N + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", what);
    hipLaunchKernelGGL((mog_lp_generic_kernel<SAMPLE>), dim3((unsigned)blocks), dim3(256), 0, st, z, params, bounds, lp,
                       g.Mz, g.Mp, g.M, g.N, D, K, ld, dr);
    return check_launch(SAMPLE ? "mog_sample (generic)" : "mog_log_prob (generic)");
}

int launch_mog_log_prob(const float* z, const float* params, const float* bounds, float* lp, int64_t Mz, int64_t Mp,
                        int64_t N, int D, int K, int64_t ld, hipStream_t st) {
    return mog_launch_forward<false>(z, params, bounds, lp, Mz, Mp, N, D, K, ld, MogDraws{nullptr, nullptr, nullptr, nullptr},
                                     st);
}

int launch_mog_sample(const float* params, const float* bounds, const float* u, const float* e1, const float* e2, float* z,
                      float* log_q, int64_t M, int64_t N, int D, int K, int64_t ld, hipStream_t st) {
    return mog_launch_forward<true>(nullptr, params, bounds, log_q, M, M, N, D, K, ld, MogDraws{u, e1, e2, z}, st);
}

// backward plan.  Shared rows keep G partial rows per context in the workspace (none when one chunk per context writes
// its own row of g_params); row per lane needs none.  The generic kernels (D = 0 instantiation) keep every workgroup's
// arrays -- prepared rows, gradient rows, per-lane vectors -- in an area of the workspace instead of LDS, so they serve
// any D and any K; at most MOG_GENERIC_WGS workgroups walk the work, which bounds the workspace.
enum { MOG_GENERIC_WGS = 512 };
struct MogBwdPlan {
    bool fused;
    int G, rc;
    int64_t blocks, area;
    size_t smem;
    float *partials, *areas;  // the workspace: partial rows (M, G, P) | the generic kernels' areas (blocks, area)
    int64_t ws_bytes;
};
static MogBwdPlan mog_bwd_plan(const MogGeom& g, int D, int K, void* ws) {
    MogBwdPlan p;
    int64_t partial_floats = 0;
    const int64_t P = mog_P(D, K), LDP = mog_ldp(D, K);
    p.fused = !g_force_generic && mog_fused_supported(D, K);
    p.G = 1, p.rc = 0;
    if (g.shared) {
        int64_t G = (g.N + MOG_TILE - 1) / MOG_TILE;
        const int64_t cap = g.M >= 256 ? 1 : 256 / g.M;
        if (G > cap) G = cap;
        p.G = G < 1 ? 1 : (int)G;
        p.area = LDP + P + 2 * D + (int64_t)MOG_TILE * ((3 * D + 2) | 1);
        p.blocks = g.M * p.G;
        if (p.G > 1) partial_floats = g.M * p.G * P;
    } else {
        const int64_t lanes = p.fused ? 0 : (int64_t)MOG_TILE * ((3 * D) | 1);
        int64_t rc = p.fused ? (MOG_LDS_FLOATS - 2 * D) / (2 * LDP) : 32768 / LDP;
        if (rc > MOG_TILE) rc = MOG_TILE;
        if (rc > 64 && rc < MOG_TILE) rc = 64;  // whole waves: no wave that carries a lane or two
        if (rc < 1) rc = 1;
        p.rc = (int)rc;
        p.area = 2 * rc * LDP + 2 * D + lanes;
        p.blocks = (g.M + rc - 1) / rc;
    }
    if (p.fused) {
        p.smem = (size_t)p.area * 4;
        p.area = 0;
    } else {
        p.smem = 0;
        if (p.blocks > MOG_GENERIC_WGS) p.blocks = MOG_GENERIC_WGS;
    }
    Carver c(ws);
    p.partials = c.take<float>(partial_floats, 16);
    p.areas = c.take<float>(p.blocks * p.area, 4);
    p.ws_bytes = c.bytes();
    return p;
}

int64_t mog_bwd_workspace(int64_t M, int64_t Mp, int64_t N, int D, int K) {
    if (mog_num_params(D, K) < 0) return -1;
    const MogGeom g = mog_geom(M, Mp, N);
    if (g.M * g.N == 0) return 0;
    return mog_bwd_plan(g, D, K, nullptr).ws_bytes;
}

#define MOG_BWD_CASE(Dv, KERNEL, ...)                                                    \
    case Dv:                                                                             \
        if (launch_lds("mog_log_prob_backward", KERNEL<Dv>, grid, dim3(MOG_TILE), pl.smem, st, __VA_ARGS__)) return TNF_ELAUNCH; \
        break;
#define MOG_BWD_SWITCH(KERNEL, ...)                                                                                  \
    switch (pl.fused ? D : 0) {                                                                                      \
        MOG_BWD_CASE(0, KERNEL, __VA_ARGS__)                                                                         \
        MOG_BWD_CASE(2, KERNEL, __VA_ARGS__) MOG_BWD_CASE(3, KERNEL, __VA_ARGS__) MOG_BWD_CASE(4, KERNEL, __VA_ARGS__) \
        MOG_BWD_CASE(5, KERNEL, __VA_ARGS__) MOG_BWD_CASE(6, KERNEL, __VA_ARGS__) MOG_BWD_CASE(7, KERNEL, __VA_ARGS__) \
        MOG_BWD_CASE(8, KERNEL, __VA_ARGS__) MOG_BWD_CASE(9, KERNEL, __VA_ARGS__) MOG_BWD_CASE(10, KERNEL, __VA_ARGS__) \
        MOG_BWD_CASE(11, KERNEL, __VA_ARGS__) MOG_BWD_CASE(12, KERNEL, __VA_ARGS__) MOG_BWD_CASE(13, KERNEL, __VA_ARGS__) \
        MOG_BWD_CASE(14, KERNEL, __VA_ARGS__) MOG_BWD_CASE(15, KERNEL, __VA_ARGS__) MOG_BWD_CASE(16, KERNEL, __VA_ARGS__) \
        default:                                                                                                     \
            return fail(TNF_EUNSUPPORTED, "mog_log_prob_backward: no kernel for D=%d", D);                           \
    }

int launch_mog_log_prob_backward(const float* z, const float* params, const float* bounds, const float* g_lp, float* g_z,
                                 float* g_params, int64_t Mz0, int64_t Mp0, int64_t N0, int D, int K, int64_t ld, void* ws,
                                 hipStream_t st) {
    const MogGeom g = mog_geom(Mz0, Mp0, N0);
    const int P = (int)mog_P(D, K);
    if (g.N == 0) {
        if (hipMemsetAsync(g_params, 0, (size_t)g.Mp * P * 4, st) != hipSuccess)
            return fail(TNF_ELAUNCH, "mog_log_prob_backward: memset failed");
        return TNF_OK;
    }
    const MogBwdPlan pl = mog_bwd_plan(g, D, K, ws);
    if (pl.blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "mog_log_prob_backward: grid too large");
    const dim3 grid((unsigned)pl.blocks);
    float* areas = pl.areas;  // used by the generic kernels only
    if (!g.shared) {
        MOG_BWD_SWITCH(mog_bwd_lane_kernel, z, params, bounds, g_lp, g_z, g_params, g.Mz, g.M, g.N, D, K, ld, pl.rc, areas,
                       pl.area)
        if (pl.fused) mog_count(TNF_MOG_COUNT_LOGPROB_BWD);
        return check_launch("mog_log_prob_backward (row per lane)");
    }
    const int G = pl.G;
    const int64_t ntiles = (g.N + MOG_TILE - 1) / MOG_TILE;
    const int64_t per = (ntiles + G - 1) / G;
    float* partial = G == 1 ? g_params : pl.partials;
    MOG_BWD_SWITCH(mog_bwd_shared_kernel, z, params, bounds, g_lp, g_z, partial, g.Mz, g.Mp, g.M, g.N, D, K, ld, G, per,
                   areas, pl.area)
    if (pl.fused) mog_count(TNF_MOG_COUNT_LOGPROB_BWD);
    int rc = check_launch("mog_log_prob_backward (shared row)");
    if (rc || G == 1) return rc;
    const int64_t blocks = (g.M * P + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "mog_log_prob_backward: grid too large");
    hipLaunchKernelGGL(mog_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)pl.partials, g_params, g.M, P, G);
    return check_launch("mog_log_prob_backward (ordered sum)");
}

}  // namespace tnf
