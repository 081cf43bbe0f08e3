// Rejection ABC on the Mat simulator (include/tnf_abc.h): ABC-SMC without resampling / ABC-MCMC with its degenerate
// Metropolis ratio are both "N independent chains, each round the first accepted candidate around the last one", so
// all T rounds of all chains run in ONE launch and no trial touches HBM (with the in-kernel stream).
//
// Layout: one wave (a workgroup of 64) owns one chain; the grid is N workgroups and the hardware scheduler balances
// chains of very different length.  A SWEEP is 64 consecutive trials, lane l evaluating trial base + l:
//   omega   D normals from the counter-based stream (abc_normals) or from the caller's block
//   z       mu + L omega, mu wave-uniform; L, the bounds and eps are read at wave-uniform addresses (scalar loads)
//   box     lb < z < ub
//   A(z)    d x d in registers, every index static (d is a template parameter, every loop unrolls)
//   det     LU with partial pivoting: the pivot is brought up by compare-and-select row swaps (a bubble pass over the
//           rows below), no dynamic indexing; trace; the two strict comparisons
// then ONE 64-bit ballot: the lowest set lane is the first accepted trial of the sweep and sweeps run in trial order,
// so the accepted trial is the first in stream order whatever the geometry.  The winner's z is broadcast (readlane) as
// the next round's mu and written by the winner's lane.  Every loop is bounded by max_trials; a chain that exhausts a
// round writes NaN rows and trials = 0 from there on.  Plain vector stores only, no atomics.
// d == 0 compiles the simulator stage out: the truncated-Gaussian draw of GaussianProposal.rvs, D = 1 .. 21.
// The libm logf / sincosf / sqrtf are used on purpose: the tests' bars are those of a float32 restatement with
// correctly-rounded-class functions, and the hardware forms of wave_prims.h do not meet them near u1 = 1.
#include <atomic>

#include "launch.h"
#include "philox.h"
#include "wave_prims.h"
#include "../../include/tnf_abc.h"

namespace tnf {

static std::atomic<long long> g_abc_launches[TNF_ABC_COUNTERS];
static void abc_count(int which) { g_abc_launches[which].fetch_add(1, std::memory_order_relaxed); }

// ---- the stream (abc_philox, abc_pair: philox.h) -----------------------------------------------------------------------
// the D normals of trial j of chain i in round t
template <int D>
__device__ __forceinline__ void abc_normals(uint32_t k0, uint32_t k1, uint32_t j, uint32_t t, uint32_t i, float (&om)[D]) {
#pragma unroll
    for (int b = 0; b < (D + 3) / 4; ++b) {
        uint32_t w[4];
        abc_philox(j, t, i, (uint32_t)b, k0, k1, w);
        float n0, n1;
        abc_pair(w[0], w[1], n0, n1);
        om[4 * b] = n0;
        if (4 * b + 1 < D) om[4 * b + 1] = n1;
        if (4 * b + 2 < D) {
            abc_pair(w[2], w[3], n0, n1);
            om[4 * b + 2] = n0;
            if (4 * b + 3 < D) om[4 * b + 3] = n1;
        }
    }
}

__global__ __launch_bounds__(256) void abc_noise_kernel(float* __restrict__ omega, uint32_t k0, uint32_t k1, uint32_t t,
                                                        uint32_t i0, int64_t n_i, uint32_t j0, int64_t n_j, int D) {
    const int nb = (D + 3) / 4;
    const int64_t total = n_i * n_j * nb;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx % nb);
    const int64_t trial = idx / nb;
    const int64_t a = trial / n_j, c = trial - a * n_j;
    uint32_t w[4];
    abc_philox(j0 + (uint32_t)c, t, i0 + (uint32_t)a, (uint32_t)b, k0, k1, w);
    float n[4];
    abc_pair(w[0], w[1], n[0], n[1]);
    abc_pair(w[2], w[3], n[2], n[3]);
    float* out = omega + trial * D;
    for (int q = 0; q < 4; ++q)
        if (4 * b + q < D) out[4 * b + q] = n[q];
}

// ---- the simulator: (det, trace) of the symmetric matrix filled row-wise from z ------------------------------------------
template <int d>
__device__ __forceinline__ void abc_mat_stats(const float* z, float& det_out, float& tr_out) {
    float a[d][d];
#pragma unroll
    for (int i = 0; i < d; ++i)
#pragma unroll
        for (int j = i; j < d; ++j) {
            const float v = z[i * d - i * (i - 1) / 2 + (j - i)];
            a[i][j] = v;
            a[j][i] = v;
        }
    float tr = a[0][0];
#pragma unroll
    for (int i = 1; i < d; ++i) tr += a[i][i];
    float det = 1.0f;
#pragma unroll
    for (int c = 0; c < d; ++c) {
#pragma unroll
        for (int r = c + 1; r < d; ++r) {  // after this pass row c holds the column's largest |entry|
            const bool sw = fabsf(a[r][c]) > fabsf(a[c][c]);
#pragma unroll
            for (int k = c; k < d; ++k) {
                const float x = a[c][k], y = a[r][k];
                a[c][k] = sw ? y : x;
                a[r][k] = sw ? x : y;
            }
            det = sw ? -det : det;
        }
        const float p = a[c][c];
        det *= p;
        const float inv = p != 0.0f ? 1.0f / p : 0.0f;  // a zero pivot: the column below is zero too, det is 0
#pragma unroll
        for (int r = c + 1; r < d; ++r) {
            const float f = a[r][c] * inv;
#pragma unroll
            for (int k = c + 1; k < d; ++k) a[r][k] -= f * a[c][k];
        }
    }
    det_out = det;
    tr_out = tr;
}

struct AbcArgs {
    const float* start;   // (Ms, D) starting points / means; Ms in {1, N}
    const float* chol;    // (D, D) lower triangle
    const float* bounds;  // (2, D)
    const float* x0;      // (2), SMC only
    const float* eps;     // (T, 2), SMC only
    const float* omega;   // NULL or (T, N, max_trials, D)
    float* zs;            // (T, N, D)
    float* xs;            // (T, N, 2), SMC only
    int32_t* trials;      // (T, N)
    uint32_t k0, k1;
    int64_t N, T;
    int start_stride;     // 0: one shared starting row
    int max_trials;
};

__device__ __forceinline__ float abc_readlane(float v, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

template <int d, int D>
__global__ __launch_bounds__(64) void abc_chain_kernel(AbcArgs a) {
    static_assert(d == 0 || D == d * (d + 1) / 2, "Mat(d) has d (d + 1) / 2 free entries");
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x + (int64_t)gridDim.x * (int64_t)blockIdx.y;
    if (i >= a.N) return;
    const float* __restrict__ chol = a.chol;
    const float* __restrict__ bounds = a.bounds;
    const float nan = __builtin_nanf("");
    float mu[D];
#pragma unroll
    for (int k = 0; k < D; ++k) mu[k] = a.start[i * a.start_stride + k];
    float x00 = 0.f, x01 = 0.f;
    if (d) x00 = a.x0[0], x01 = a.x0[1];
    bool alive = true;
    for (int64_t t = 0; t < a.T; ++t) {
        const int64_t row = t * a.N + i;
        int won = 0;
        if (alive) {
            float e0 = 0.f, e1 = 0.f;
            if (d) e0 = a.eps[2 * t], e1 = a.eps[2 * t + 1];
            const float* om_row = a.omega ? a.omega + row * (int64_t)a.max_trials * D : nullptr;
            for (int base = 0; base < a.max_trials; base += 64) {
                const int j = base + lane;
                const bool valid = j < a.max_trials;
                float om[D];
                if (om_row) {
#pragma unroll
                    for (int k = 0; k < D; ++k) om[k] = valid ? om_row[(int64_t)j * D + k] : 0.0f;
                } else {
                    abc_normals<D>(a.k0, a.k1, (uint32_t)j, (uint32_t)t, (uint32_t)i, om);
                }
                float z[D];
                bool ok = valid;
#pragma unroll
                for (int r = 0; r < D; ++r) {
                    float acc = mu[r];
#pragma unroll
                    for (int k = 0; k <= r; ++k) acc = fmaf(chol[r * D + k], om[k], acc);
                    z[r] = acc;
                    ok = ok && (bounds[r] < acc) && (acc < bounds[D + r]);
                }
                float det = 0.f, tr = 0.f;
                if constexpr (d > 0) {
                    abc_mat_stats<d>(z, det, tr);
                    ok = ok && (fabsf(det - x00) < e0) && (fabsf(tr - x01) < e1);
                }
                const unsigned long long mask = __ballot(ok);
                if (mask) {
                    const int win = __ffsll((long long)mask) - 1;
                    won = base + win + 1;
                    if (lane == win) {
#pragma unroll
                        for (int k = 0; k < D; ++k) a.zs[row * D + k] = z[k];
                        if (d) a.xs[row * 2] = det, a.xs[row * 2 + 1] = tr;
                        a.trials[row] = won;
                    }
#pragma unroll
                    for (int k = 0; k < D; ++k) mu[k] = abc_readlane(z[k], win);
                    break;
                }
            }
            alive = won != 0;
        }
        if (!won) {
            if (lane < D) a.zs[row * D + lane] = nan;
            if (d && lane < 2) a.xs[row * 2 + lane] = nan;
            if (lane == 0) a.trials[row] = 0;
        }
    }
}

static dim3 abc_grid(int64_t N) {  // N < 2^24 workgroups, x alone would do; kept two-dimensional like grid_xm
    const int64_t gx = N < 65536 ? N : 65536;
    return dim3((unsigned)gx, (unsigned)((N + gx - 1) / gx));
}

static int abc_check_common(const char* fn, int64_t N, int32_t max_trials) {
    if (N < 0 || N >= (1 << 24)) return fail(TNF_EINVAL, "%s: %lld chains, the limit is 2^24 - 1", fn, (long long)N);
    if (max_trials < 1 || max_trials > TNF_ABC_MAX_TRIALS)
        return fail(TNF_EINVAL, "%s: max_trials=%d, must be 1 .. %d", fn, max_trials, TNF_ABC_MAX_TRIALS);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_abc_supported(int32_t d) { return d >= 2 && d <= TNF_ABC_MAX_SMC_D ? 1 : 0; }

int64_t tnf_abc_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_ABC_COUNTERS) return fail(TNF_EINVAL, "tnf_abc_launch_count: counter %d", which);
    return g_abc_launches[which].load(std::memory_order_relaxed);
}

int tnf_abc_smc_mat_f32(const float* z0, const float* chol, const float* bounds, const float* x0, const float* eps,
                        const float* omega, float* zs, float* xs, int32_t* trials, int64_t seed, int64_t N, int64_t T,
                        int32_t d, int32_t max_trials, void* stream) {
    const char* fn = "tnf_abc_smc_mat_f32";
    if (!tnf_abc_supported(d)) return fail(TNF_EUNSUPPORTED, "%s: d=%d, the kernel exists for 2 <= d <= %d", fn, d, TNF_ABC_MAX_SMC_D);
    if (int rc = abc_check_common(fn, N, max_trials)) return rc;
    if (T < 0 || T > 0x7fffffffLL) return fail(TNF_EINVAL, "%s: T=%lld rounds, the limit is 2^31 - 1", fn, (long long)T);
    if (!z0 || !chol || !bounds || !x0 || !eps || !zs || !xs || !trials) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (N == 0 || T == 0) return TNF_OK;
    const int D = d * (d + 1) / 2;
    const AbcArgs a{z0, chol, bounds, x0, eps, omega, zs, xs, trials, (uint32_t)((uint64_t)seed & 0xffffffffu),
                    (uint32_t)((uint64_t)seed >> 32), N, T, D, max_trials};
    dispatch_range<2, TNF_ABC_MAX_SMC_D>(d, [&](auto dc) {
        constexpr int dv = decltype(dc)::value;
        hipLaunchKernelGGL((abc_chain_kernel<dv, dv * (dv + 1) / 2>), abc_grid(N), dim3(64), 0, as_stream(stream), a);
        return 0;
    });
    abc_count(TNF_ABC_COUNT_SMC);
    return check_launch(fn);
}

int tnf_abc_propose_f32(const float* mu, const float* chol, const float* bounds, const float* omega, float* z,
                        int32_t* trials, int64_t seed, int64_t M, int64_t M_mu, int32_t D, int32_t max_trials, void* stream) {
    const char* fn = "tnf_abc_propose_f32";
    if (D < 1 || D > TNF_ABC_MAX_D) return fail(TNF_EUNSUPPORTED, "%s: D=%d, the kernel exists for 1 <= D <= %d", fn, D, TNF_ABC_MAX_D);
    if (int rc = abc_check_common(fn, M, max_trials)) return rc;
    if (M_mu != 1 && M_mu != M) return fail(TNF_EINVAL, "%s: M_mu=%lld must be 1 or M=%lld", fn, (long long)M_mu, (long long)M);
    if (!mu || !chol || !bounds || !z || !trials) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (M == 0) return TNF_OK;
    const AbcArgs a{mu, chol, bounds, nullptr, nullptr, omega, z, nullptr, trials, (uint32_t)((uint64_t)seed & 0xffffffffu),
                    (uint32_t)((uint64_t)seed >> 32), M, 1, M_mu == 1 ? 0 : D, max_trials};
    dispatch_range<1, TNF_ABC_MAX_D>(D, [&](auto Dc) {
        hipLaunchKernelGGL((abc_chain_kernel<0, decltype(Dc)::value>), abc_grid(M), dim3(64), 0, as_stream(stream), a);
        return 0;
    });
    abc_count(TNF_ABC_COUNT_PROPOSE);
    return check_launch(fn);
}

int tnf_abc_noise_f32(float* omega, int64_t seed, int64_t t, int64_t i0, int64_t n_i, int64_t j0, int64_t n_j, int32_t D,
                      void* stream) {
    const char* fn = "tnf_abc_noise_f32";
    if (D < 1 || D > TNF_ABC_MAX_D) return fail(TNF_EUNSUPPORTED, "%s: D=%d, the stream serves 1 <= D <= %d", fn, D, TNF_ABC_MAX_D);
    if (t < 0 || t > 0x7fffffffLL || i0 < 0 || n_i < 0 || j0 < 0 || n_j < 0 || i0 + n_i > (1 << 24) || j0 + n_j > (1 << 24))
        return fail(TNF_EINVAL, "%s: t=%lld i0=%lld n_i=%lld j0=%lld n_j=%lld outside the stream's counters", fn, (long long)t,
                    (long long)i0, (long long)n_i, (long long)j0, (long long)n_j);
    if (!omega) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (n_i == 0 || n_j == 0) return TNF_OK;
    const int64_t blocks = (n_i * n_j * ((D + 3) / 4) + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
    hipLaunchKernelGGL(abc_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), omega,
                       (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), (uint32_t)t, (uint32_t)i0, n_i,
                       (uint32_t)j0, n_j, (int)D);
    abc_count(TNF_ABC_COUNT_NOISE);
    return check_launch(fn);
}

}  // extern "C"
