// The EFN training loop's two host round trips as kernels (include/tnf_efn.h): the prior over natural parameters and the
// per-context KL diagnostic.
//
// Prior, MVN: one wave per context.  The D + D(D-1)/2 head normals (mu, strict lower triangle of the Bartlett factor L) go
// straight into LDS; each diagonal entry is the square root of a sum of df - i squared normals, a Philox block (four
// normals) per lane and step, every lane adding its own draws in increasing k and the 64 lane sums combined by an xor
// butterfly (a + b commutes: the same bits in every lane, and the association is a function of (D, df) alone).  Then
// W = L L^T / df row by row, a lane per column, and eta1 = W mu; nothing is inverted.  A recorded noise row replaces the
// stream at the one place where a block is fetched (efn_block4), so both modes run the same arithmetic on the same bits.
// Prior, Dirichlet and the noise entry: a Philox block per thread.
//
// KL: prepare (one wave per context: Cholesky of the precision in LDS, two triangular solves with the running vector in
// registers and its pivot entry broadcast by a shuffle), stream (the structure of ef_dot_mvn_kernel<D>: a 128-sample tile
// staged through LDS with an odd row stride, one sample per lane, the prepared row -- wave-uniform -- on scalar loads
// feeding the FMAs), reduce (ordered).  log_q - log p is added in double: per lane in tile order, the workgroup's 128 lane
// sums by a fixed LDS tree, the workgroups' partials in workgroup order -- no float atomics, bit-reproducible.
// Plain vector stores only.  libm logf / sincosf / lgamma, for the reason abc_kernels.hip gives.
#include <atomic>
#include <cmath>

#include "launch.h"
#include "philox.h"
#include "../../include/tnf_efn.h"

namespace tnf {

static std::atomic<long long> g_efn_launches[TNF_EFN_COUNTERS];
static void efn_count(int which) { g_efn_launches[which].fetch_add(1, std::memory_order_relaxed); }

enum { EFN_LD = TNF_EFN_MAX_D + 1, EFN_TILE = 128 };

struct EfnPriorArgs {
    float* eta;            // (M, D_eta)
    const float* noise;    // NULL or (M, K)
    const int64_t* t_dev;  // NULL or the draw index on the device
    uint32_t k0, k1, t, i0;
    int64_t M;
    int D, df;
    float sigma_mu, lb, ub;
};

// draws 4b .. 4b + 3 of one context: from its recorded row (entries at K and beyond read as 0) or from the stream
template <bool NORMAL>
__device__ __forceinline__ void efn_block4(const float* row, int K, uint32_t b, uint32_t t, uint32_t ctx, uint32_t k0,
                                           uint32_t k1, float (&v)[4]) {
    if (row) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (int)(4 * b) + c < K ? row[4 * b + c] : 0.0f;
        return;
    }
    uint32_t w[4];
    abc_philox(b, t, ctx, NORMAL ? TNF_EFN_PURPOSE_NORMAL : TNF_EFN_PURPOSE_UNIFORM, k0, k1, w);
    if constexpr (NORMAL) {
        abc_pair(w[0], w[1], v[0], v[1]);
        abc_pair(w[2], w[3], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = ((float)(w[c] >> 8) + 0.5f) * 0x1p-24f;
    }
}

__device__ __forceinline__ float efn_wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(64) void efn_prior_mvn_kernel(EfnPriorArgs a) {
    __shared__ float Ls[TNF_EFN_MAX_D * EFN_LD];  // the Bartlett factor, lower triangle
    __shared__ float Ws[TNF_EFN_MAX_D * EFN_LD];  // W = L L^T / df, both triangles
    __shared__ float mus[TNF_EFN_MAX_D];
    const int64_t m = grid_m();
    if (m >= a.M) return;
    const int lane = threadIdx.x;
    const int D = a.D, df = a.df;
    const int head = D + D * (D - 1) / 2;
    const int K = D * (1 + df);
    const int Deta = D + D * (D + 1) / 2;
    const uint32_t t = a.t_dev ? (uint32_t)*a.t_dev : a.t;
    const uint32_t ctx = a.i0 + (uint32_t)m;
    const float* row = a.noise ? a.noise + m * K : nullptr;
    float* eta = a.eta + m * Deta;
    float v[4];
    for (int b = lane; 4 * b < head; b += 64) {
        efn_block4<true>(row, K, (uint32_t)b, t, ctx, a.k0, a.k1, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 4 * b + c;
            if (k < D) {
                mus[k] = __fmul_rn(a.sigma_mu, v[c]);
            } else if (k < head) {
                const int p = k - D;  // row i of the strict lower triangle starts at i (i - 1) / 2
                int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
                while (i * (i - 1) / 2 > p) --i;
                while ((i + 1) * i / 2 <= p) ++i;
                Ls[i * EFN_LD + (p - i * (i - 1) / 2)] = v[c];
            }
        }
    }
    for (int i = 0; i < D; ++i) {
        const int s = head + i * df - i * (i - 1) / 2, e = s + df - i;
        float acc = 0.0f;
        for (int b = s / 4 + lane; 4 * b < e; b += 64) {
            efn_block4<true>(row, K, (uint32_t)b, t, ctx, a.k0, a.k1, v);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int k = 4 * b + c;
                if (k >= s && k < e) acc = fmaf(v[c], v[c], acc);
            }
        }
        acc = efn_wave_sum(acc);
        if (lane == 0) Ls[i * EFN_LD + i] = sqrtf(acc);
    }
    __syncthreads();
    const float dff = (float)df;
    for (int i = 0; i < D; ++i) {
        const int j = lane;
        if (j >= i && j < D) {
            float acc = 0.0f;
            for (int k = 0; k <= i; ++k) acc = fmaf(Ls[i * EFN_LD + k], Ls[j * EFN_LD + k], acc);
            const float w = __fdiv_rn(acc, dff);
            Ws[i * EFN_LD + j] = w;
            Ws[j * EFN_LD + i] = w;
            eta[D + i * D - i * (i - 1) / 2 + (j - i)] = i == j ? -0.5f * w : -w;
        }
    }
    __syncthreads();
    if (lane < D) {
        float acc = 0.0f;
        for (int j = 0; j < D; ++j) acc = fmaf(Ws[lane * EFN_LD + j], mus[j], acc);
        eta[lane] = acc;
    }
}

__global__ __launch_bounds__(256) void efn_prior_dirichlet_kernel(EfnPriorArgs a) {
    const int D = a.D;
    const int nb = (D + 3) / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.M * nb) return;
    const int64_t m = idx / nb;
    const int b = (int)(idx - m * nb);
    const uint32_t t = a.t_dev ? (uint32_t)*a.t_dev : a.t;
    float v[4];
    efn_block4<false>(a.noise ? a.noise + m * D : nullptr, D, (uint32_t)b, t, a.i0 + (uint32_t)m, a.k0, a.k1, v);
    float* eta = a.eta + m * (D + 1);
    const float width = __fsub_rn(a.ub, a.lb);
    for (int c = 0; c < 4; ++c)
        if (4 * b + c < D) eta[4 * b + c] = fmaf(width, v[c], a.lb);
    if (b == 0) eta[D] = 1.0f;
}

template <bool NORMAL>
__global__ __launch_bounds__(256) void efn_noise_kernel(float* __restrict__ noise, const int64_t* t_dev, uint32_t k0,
                                                        uint32_t k1, uint32_t t, uint32_t i0, int64_t M, int K) {
    const int nb = (K + 3) / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * nb) return;
    const int64_t m = idx / nb;
    const int b = (int)(idx - m * nb);
    if (t_dev) t = (uint32_t)*t_dev;
    float v[4];
    efn_block4<NORMAL>(nullptr, K, (uint32_t)b, t, i0 + (uint32_t)m, k0, k1, v);
    float* out = noise + m * K;
    for (int c = 0; c < 4; ++c)
        if (4 * b + c < K) out[4 * b + c] = v[c];
}

// ---------------------------------------------------------------------------------------------------------------------
// KL
// ---------------------------------------------------------------------------------------------------------------------
// one wave per context: eta[m] -> prep[m] = [mu | C^T packed | const] (MVN), [alpha - 1 | const] (Dirichlet)
__global__ __launch_bounds__(64) void efn_kl_prepare_mvn_kernel(const float* __restrict__ eta, float* __restrict__ prep,
                                                                int64_t M, int D) {
    __shared__ float Cs[TNF_EFN_MAX_D * EFN_LD];
    const int64_t m = grid_m();
    if (m >= M) return;
    const int lane = threadIdx.x;
    const int Deta = D + D * (D + 1) / 2;
    const float* e = eta + m * Deta;
    float* out = prep + m * (Deta + 1);
    bool bad = false;  // the same in every lane: the pivots are broadcast
    // the precision, lower triangle: P[i][j] = P[j][i], packed entry (j, i) of row j <= i
    for (int j = 0; j < D; ++j) {
        const int i = lane;
        if (i >= j && i < D) {
            const float u = e[D + j * D - j * (j - 1) / 2 + (i - j)];
            Cs[i * EFN_LD + j] = i == j ? -2.0f * u : -u;
        }
    }
    __syncthreads();
    // left-looking Cholesky: column j from the finished columns k < j, a lane per row (a step reads those columns and
    // the lane's own entry of column j, and writes column j only: one barrier per step)
    for (int j = 0; j < D; ++j) {
        const int i = lane;
        float s = 0.0f;
        if (i >= j && i < D) {
            s = Cs[i * EFN_LD + j];
            for (int k = 0; k < j; ++k) s = fmaf(-Cs[i * EFN_LD + k], Cs[j * EFN_LD + k], s);
        }
        const float pivot = __shfl(s, j, 64);
        const float cjj = sqrtf(pivot);
        bad = bad || !(pivot > 0.0f) || !(pivot <= 3.4028234e38f);
        if (i == j) Cs[i * EFN_LD + j] = cjj;
        if (i > j && i < D) Cs[i * EFN_LD + j] = __fdiv_rn(s, cjj);
        __syncthreads();
    }
    // C y = eta1 (forward), C^T mu = y (backward): lane i keeps entry i
    float b = lane < D ? e[lane] : 0.0f;
    float y = 0.0f;
    for (int j = 0; j < D; ++j) {
        const float yj = __fdiv_rn(__shfl(b, j, 64), Cs[j * EFN_LD + j]);
        if (lane == j) y = yj;
        if (lane > j && lane < D) b = fmaf(-Cs[lane * EFN_LD + j], yj, b);
    }
    float mu = 0.0f;
    for (int j = D - 1; j >= 0; --j) {
        const float mj = __fdiv_rn(__shfl(y, j, 64), Cs[j * EFN_LD + j]);
        if (lane == j) mu = mj;
        if (lane < j) y = fmaf(-Cs[j * EFN_LD + lane], mj, y);
    }
    if (lane < D) out[lane] = mu;
    for (int i = 0; i < D; ++i) {  // row i of C^T: C[j][i], j >= i
        const int j = lane;
        if (j >= i && j < D) out[D + i * D - i * (i - 1) / 2 + (j - i)] = Cs[j * EFN_LD + i];
    }
    if (lane == 0) {
        double c = -0.5 * (double)D * 1.8378770664093454835606594728112;  // log(2 pi)
        for (int i = 0; i < D; ++i) c += log((double)Cs[i * EFN_LD + i]);
        out[Deta] = bad ? __builtin_nanf("") : (float)c;
    }
}

__global__ __launch_bounds__(64) void efn_kl_prepare_dirichlet_kernel(const float* __restrict__ eta,
                                                                      float* __restrict__ prep, int64_t M, int D) {
    __shared__ double lg[TNF_EFN_MAX_D];
    __shared__ double al[TNF_EFN_MAX_D];
    const int64_t m = grid_m();
    if (m >= M) return;
    const int lane = threadIdx.x;
    const float* e = eta + m * (D + 1);
    float* out = prep + m * (D + 2);
    if (lane < D) {
        const float a = e[lane];
        out[lane] = a - 1.0f;
        al[lane] = (double)a;
        lg[lane] = a > 0.0f ? lgamma((double)a) : (double)__builtin_nanf("");
    }
    __syncthreads();
    if (lane == 0) {
        double sa = 0.0, sl = 0.0;
        for (int d = 0; d < D; ++d) {
            sa += al[d];
            sl += lg[d];
        }
        out[D] = (float)(lgamma(sa) - sl);
        out[D + 1] = 0.0f;  // the row has D_eta + 1 entries in both families
    }
}

// the workgroup's sum of 128 lane sums, in a fixed order; valid in thread 0
__device__ __forceinline__ double efn_block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = EFN_TILE / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ void efn_stage(float* tile, const float* __restrict__ src, int nr, int D, int LD, int tid) {
    for (int idx = tid; idx < nr * D; idx += EFN_TILE) {
        const int r = idx / D, d = idx - r * D;
        tile[r * LD + d] = src[idx];
    }
}

__device__ __forceinline__ double efn_log_q(const void* log_q, int lq64, int64_t idx) {
    return lq64 ? reinterpret_cast<const double*>(log_q)[idx] : (double)reinterpret_cast<const float*>(log_q)[idx];
}

template <int D>
__global__ void __launch_bounds__(EFN_TILE)
efn_kl_mvn_kernel(const float* __restrict__ z, const void* __restrict__ log_q, int lq64, const float* __restrict__ prep,
                  double* __restrict__ partial, int64_t M, int64_t N, int64_t tiles_per_wg, int G) {
    constexpr int LD = D | 1;
    constexpr int Deta = D + D * (D + 1) / 2;
    __shared__ float tile[EFN_TILE * LD];
    __shared__ double red[EFN_TILE];
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const float* __restrict__ e = prep + m * (Deta + 1);
    const float* zm = z + m * N * D;
    double sum = 0.0;
    for (int64_t t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * EFN_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)EFN_TILE ? (N - n0) : (int64_t)EFN_TILE);
        __syncthreads();
        efn_stage(tile, zm + n0 * D, nr, D, LD, tid);
        __syncthreads();
        if (tid < nr) {
            float d[D];
#pragma unroll
            for (int j = 0; j < D; ++j) d[j] = tile[tid * LD + j] - e[j];
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int base = D + i * D - i * (i - 1) / 2 - i;  // C^T[i][j] = e[base + j]
                float y = e[base + i] * d[i];
#pragma unroll
                for (int j = i + 1; j < D; ++j) y = fmaf(e[base + j], d[j], y);
                acc = fmaf(y, y, acc);
            }
            const float log_p = fmaf(-0.5f, acc, e[Deta]);
            sum += efn_log_q(log_q, lq64, m * N + n0 + tid) - (double)log_p;
        }
    }
    const double total = efn_block_sum(sum, red, tid);
    if (tid == 0) partial[m * G + blockIdx.x] = total;
}

__global__ void __launch_bounds__(EFN_TILE)
efn_kl_dirichlet_kernel(const float* __restrict__ z, const void* __restrict__ log_q, int lq64,
                        const float* __restrict__ prep, double* __restrict__ partial, int64_t M, int64_t N, int D,
                        int64_t tiles_per_wg, int G) {
    __shared__ float tile[EFN_TILE * EFN_LD];
    __shared__ double red[EFN_TILE];
    const int LD = D | 1;
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const float* __restrict__ e = prep + m * (D + 2);
    const float* zm = z + m * N * D;
    double sum = 0.0;
    for (int64_t t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * EFN_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)EFN_TILE ? (N - n0) : (int64_t)EFN_TILE);
        __syncthreads();
        efn_stage(tile, zm + n0 * D, nr, D, LD, tid);
        __syncthreads();
        if (tid < nr) {
            float s = 0.0f;
            for (int d = 0; d < D; ++d) s += tile[tid * LD + d] + 1e-32f;
            float acc = e[D];
            for (int d = 0; d < D; ++d) acc = fmaf(e[d], logf(__fdiv_rn(tile[tid * LD + d] + 1e-32f, s)), acc);
            sum += efn_log_q(log_q, lq64, m * N + n0 + tid) - (double)acc;
        }
    }
    const double total = efn_block_sum(sum, red, tid);
    if (tid == 0) partial[m * G + blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
efn_kl_reduce_kernel(const double* __restrict__ partial, float* __restrict__ kl, int64_t M, int64_t N, int G) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double acc = 0.0;
    for (int c = 0; c < G; ++c) acc += partial[m * G + c];
    kl[m] = (float)(acc / (double)N);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static int64_t efn_num_eta(int family, int D) { return family == TNF_EF_MVN ? D + (int64_t)D * (D + 1) / 2 : D + 1; }

// workgroups per context of the KL stream kernel and the tiles each of them walks: a function of (M, N) alone
static int efn_kl_chunks(int64_t M, int64_t N, int64_t* per_out) {
    const int64_t tiles = (N + EFN_TILE - 1) / EFN_TILE;
    const int64_t want = 8192 / (M < 8192 ? (M < 1 ? 1 : M) : 8192);
    const int64_t per = (tiles + want - 1) / want < 1 ? 1 : (tiles + want - 1) / want;
    *per_out = per;
    const int64_t G = (tiles + per - 1) / per;
    return (int)(G < 1 ? 1 : G);
}

static int efn_check_stream(const char* fn, int64_t t, int64_t i0, int64_t M) {
    if (t < 0 || t > 0x7fffffffLL || i0 < 0 || M < 0 || i0 > (1LL << 31) || M > (1LL << 31) || i0 + M > (1LL << 31))
        return fail(TNF_EINVAL, "%s: t=%lld i0=%lld M=%lld outside the stream's counters", fn, (long long)t, (long long)i0,
                    (long long)M);
    return TNF_OK;
}

// the checks of (family, D, iw_df_fac) shared by the prior and the noise entry
static int efn_check_family(const char* fn, int family, int D, int iw_df_fac) {
    if (!tnf_efn_supported(family, D))
        return fail(TNF_EUNSUPPORTED, "%s: family=%d D=%d, the kernels exist for MVN and Dirichlet, 1 <= D <= %d", fn, family, D,
                    TNF_EFN_MAX_D);
    if (family == TNF_EF_MVN) {
        if (iw_df_fac < 1) return fail(TNF_EINVAL, "%s: iw_df_fac=%d, must be at least 1", fn, iw_df_fac);
        if ((int64_t)iw_df_fac * D > TNF_EFN_MAX_DF)
            return fail(TNF_EINVAL, "%s: df=%lld, the chi-square sums serve df <= %d", fn, (long long)iw_df_fac * D,
                        TNF_EFN_MAX_DF);
    }
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_efn_supported(int32_t family, int32_t D) {
    return (family == TNF_EF_MVN || family == TNF_EF_DIRICHLET) && D >= 1 && D <= TNF_EFN_MAX_D ? 1 : 0;
}

int64_t tnf_efn_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_EFN_COUNTERS) return fail(TNF_EINVAL, "tnf_efn_launch_count: counter %d", which);
    return g_efn_launches[which].load(std::memory_order_relaxed);
}

int64_t tnf_efn_prior_num_noise(int32_t family, int32_t D, int32_t iw_df_fac) {
    if (efn_check_family("tnf_efn_prior_num_noise", family, D, iw_df_fac)) return -1;
    return family == TNF_EF_MVN ? (int64_t)D * (1 + (int64_t)iw_df_fac * D) : (int64_t)D;
}

int tnf_efn_prior_noise_f32(float* noise, const int64_t* t_dev, int32_t family, int32_t D, int32_t iw_df_fac, int64_t seed,
                            int64_t t, int64_t i0, int64_t M, void* stream) {
    const char* fn = "tnf_efn_prior_noise_f32";
    if (int rc = efn_check_family(fn, family, D, iw_df_fac)) return rc;
    if (int rc = efn_check_stream(fn, t, i0, M)) return rc;
    if (!noise) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (M == 0) return TNF_OK;
    const int K = (int)tnf_efn_prior_num_noise(family, D, iw_df_fac);
    const int64_t blocks = (M * ((K + 3) / 4) + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
    dispatch_bool(family == TNF_EF_MVN, [&](auto normal) {
        hipLaunchKernelGGL(efn_noise_kernel<decltype(normal)::value>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                           noise, t_dev, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32),
                           (uint32_t)t, (uint32_t)i0, M, K);
        return 0;
    });
    efn_count(TNF_EFN_COUNT_NOISE);
    return check_launch(fn);
}

int tnf_efn_prior_f32(float* eta, const float* noise, const int64_t* t_dev, int32_t family, int32_t D, int32_t iw_df_fac,
                      float sigma_mu, float lb, float ub, int64_t seed, int64_t t, int64_t i0, int64_t M, void* stream) {
    const char* fn = "tnf_efn_prior_f32";
    if (int rc = efn_check_family(fn, family, D, iw_df_fac)) return rc;
    if (!eta) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (family == TNF_EF_MVN) {
        if (!(sigma_mu >= 0.0f)) return fail(TNF_EINVAL, "%s: sigma_mu=%g, must be >= 0", fn, (double)sigma_mu);
    } else if (!std::isfinite(lb) || !std::isfinite(ub) || lb > ub) {
        return fail(TNF_EINVAL, "%s: lb=%g ub=%g, must be finite with lb <= ub", fn, (double)lb, (double)ub);
    }
    if (int rc = efn_check_stream(fn, t, i0, M)) return rc;
    if (M == 0) return TNF_OK;
    const EfnPriorArgs a{eta, noise, t_dev, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32),
                         (uint32_t)t, (uint32_t)i0, M, D, family == TNF_EF_MVN ? iw_df_fac * D : 0, sigma_mu, lb, ub};
    if (family == TNF_EF_MVN) {
        hipLaunchKernelGGL(efn_prior_mvn_kernel, grid_xm(1, M), dim3(64), 0, as_stream(stream), a);
    } else {
        const int64_t blocks = (M * ((D + 3) / 4) + 255) / 256;
        if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
        hipLaunchKernelGGL(efn_prior_dirichlet_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a);
    }
    efn_count(TNF_EFN_COUNT_PRIOR);
    return check_launch(fn);
}

int64_t tnf_efn_kl_workspace_bytes(int32_t family, int64_t M, int64_t N, int32_t D) {
    if (!tnf_efn_supported(family, D) || M < 0 || N < 1 || M > (1LL << 31)) return -1;
    int64_t per;
    const int G = efn_kl_chunks(M, N, &per);
    return M * ((int64_t)G * 8 + (efn_num_eta(family, D) + 1) * 4);
}

int tnf_efn_kl_f32(const float* z, const void* log_q, int32_t log_q_dtype, const float* eta, float* kl, int32_t family,
                   int64_t M, int64_t N, int32_t D, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_efn_kl_f32";
    if (!tnf_efn_supported(family, D))
        return fail(TNF_EUNSUPPORTED, "%s: family=%d D=%d, the kernels exist for MVN and Dirichlet, 1 <= D <= %d", fn, family, D,
                    TNF_EFN_MAX_D);
    if (!z || !log_q || !eta || !kl || !workspace) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (log_q_dtype != TNF_F32 && log_q_dtype != TNF_F64)
        return fail(TNF_EINVAL, "%s: log_q_dtype=%d, must be TNF_F32 or TNF_F64", fn, log_q_dtype);
    if (M < 0 || N < 1 || M > (1LL << 31))
        return fail(TNF_EINVAL, "%s: M=%lld N=%lld, need 0 <= M <= 2^31 and N >= 1", fn, (long long)M, (long long)N);
    const int64_t need = tnf_efn_kl_workspace_bytes(family, M, N, D);
    if (workspace_bytes < need)
        return fail(TNF_EWORKSPACE, "%s: workspace of %lld B, %lld B needed", fn, (long long)workspace_bytes, (long long)need);
    if (M == 0) return TNF_OK;
    int64_t per;
    const int G = efn_kl_chunks(M, N, &per);
    double* partial = reinterpret_cast<double*>(workspace);
    float* prep = reinterpret_cast<float*>(partial + M * G);
    hipStream_t st = as_stream(stream);
    const int lq64 = log_q_dtype == TNF_F64;
    if (family == TNF_EF_MVN) {
        hipLaunchKernelGGL(efn_kl_prepare_mvn_kernel, grid_xm(1, M), dim3(64), 0, st, eta, prep, M, (int)D);
        dispatch_range<1, TNF_EFN_MAX_D>(D, [&](auto dc) {
            hipLaunchKernelGGL(efn_kl_mvn_kernel<decltype(dc)::value>, grid_xm(G, M), dim3(EFN_TILE), 0, st, z, log_q, lq64,
                               (const float*)prep, partial, M, N, per, G);
            return 0;
        });
    } else {
        hipLaunchKernelGGL(efn_kl_prepare_dirichlet_kernel, grid_xm(1, M), dim3(64), 0, st, eta, prep, M, (int)D);
        hipLaunchKernelGGL(efn_kl_dirichlet_kernel, grid_xm(G, M), dim3(EFN_TILE), 0, st, z, log_q, lq64, (const float*)prep,
                           partial, M, N, (int)D, per, G);
    }
    hipLaunchKernelGGL(efn_kl_reduce_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const double*)partial, kl,
                       M, N, G);
    efn_count(TNF_EFN_COUNT_KL);
    return check_launch(fn);
}

}  // extern "C"
