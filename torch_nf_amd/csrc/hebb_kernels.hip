// The Hebbian learning-rule simulator (include/tnf_hebb.h): n_steps dependent steps of a rank-one weight update with
// fresh Gaussian noise, for N independent parameter sets, in ONE launch; the state never leaves registers.
//
// Layout: a simulation is owned by a GROUP of G lanes, G = ceil(n / 4) rounded up to a power of two (1 .. 16); lane q of
// the group holds neurons 4q .. 4q + 3, so its noise for one step is exactly one Philox block (counter word 3 = q) and
// no round is computed twice.  Groups are G-aligned inside a wave, 64 / G simulations per wave.  Per step:
//   x row   the shared inputs are staged once per workgroup in LDS, rows padded with zeros to 4G floats: one
//           ds_read_b128 per lane (a table too large for LDS is read from global memory, same values)
//   y       four FMAs per lane, then log2(G) DPP steps inside the group (quad_perm xor 1, xor 2, row_half_mirror,
//           row_mirror): a + b is commutative, so every lane of the group holds the same bits, and the association is a
//           function of n alone -- never of the lane, wave or launch that owns the simulation
//   update  every operation rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn: no contraction), then the two
//           compare-and-select clips; tail neurons (k >= n) are held at 0 and multiply a zero of the padded x row
//   traj    the only per-step store
// Lanes of a group beyond ceil(n / 4) (n = 20: 3 of 8) carry zeros; they cost issue slots, not correctness.
// Plain vector stores only, no atomics.  libm logf / sincosf inside abc_pair (philox.h), for the reason abc_kernels.hip
// gives.
#include <atomic>

#include "launch.h"
#include "philox.h"
#include "wave_prims.h"
#include "../../include/tnf_hebb.h"

namespace tnf {

static std::atomic<long long> g_hebb_launches[TNF_HEBB_COUNTERS];
static void hebb_count(int which) { g_hebb_launches[which].fetch_add(1, std::memory_order_relaxed); }

struct HebbArgs {
    const float* z;        // (N, 4)
    const float* x;        // (N_x, n)
    const float* w0;       // (N_w0, n)
    const float* eps;      // NULL or (n_steps, N, n)
    float* w;              // (N, n)
    float* traj;           // NULL or (n_steps, N, n)
    const int64_t* t_dev;  // NULL or the draw index on the device
    uint32_t k0, k1, t, i0, j0;
    int64_t N, n_steps;
    int w0_stride;         // 0: one shared starting row
    int n, N_x;
    float sigma;
};

template <int CTRL>
__device__ __forceinline__ float hebb_dpp(float v) {
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}

// sum over the G lanes of a group; the same bits in every lane of the group
template <int G>
__device__ __forceinline__ float hebb_group_sum(float v) {
    if constexpr (G >= 2) v += hebb_dpp<0xB1>(v);    // quad_perm [1, 0, 3, 2]: lane ^ 1
    if constexpr (G >= 4) v += hebb_dpp<0x4E>(v);    // quad_perm [2, 3, 0, 1]: lane ^ 2
    if constexpr (G >= 8) v += hebb_dpp<0x141>(v);   // row_half_mirror: the other quad of the 8 (its lanes agree by now)
    if constexpr (G >= 16) v += hebb_dpp<0x140>(v);  // row_mirror: the other half of the 16
    return v;
}

template <int G, bool LDSX>
__global__ __launch_bounds__(256) void hebb_sim_kernel(HebbArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hebb_xs[];  // (N_x, 4G), zero-padded rows
    constexpr int W = 4 * G;
    const int n = a.n;
    if constexpr (LDSX) {
        for (int idx = threadIdx.x; idx < a.N_x * W; idx += blockDim.x) {
            const int r = idx / W, k = idx - r * W;
            hebb_xs[idx] = k < n ? a.x[r * n + k] : 0.0f;
        }
        __syncthreads();
    }
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid / G;
    const int q = (int)(gid % G);
    if (i >= a.N) return;  // whole groups leave: no lane of a live group reads a dead one
    const uint32_t t = a.t_dev ? (uint32_t)*a.t_dev : a.t;
    const float alpha = a.z[4 * i], beta = a.z[4 * i + 1], theta = a.z[4 * i + 2], b = a.z[4 * i + 3];
    const float nb = -b;
    bool live[4];
    float w[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        live[c] = 4 * q + c < n;
        w[c] = live[c] ? a.w0[i * a.w0_stride + 4 * q + c] : 0.0f;
    }
    int xr = (int)(a.j0 % (uint32_t)a.N_x);
    const int64_t row_step = a.N * n;  // floats between two steps of eps / traj
    int64_t off = i * n + 4 * q;       // this lane's four entries of step 0
    for (int64_t s = 0; s < a.n_steps; ++s) {
        float xv[4];
        if constexpr (LDSX) {
            const f4 v = *reinterpret_cast<const f4*>(&hebb_xs[xr * W + 4 * q]);
            xv[0] = v[0], xv[1] = v[1], xv[2] = v[2], xv[3] = v[3];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) xv[c] = live[c] ? a.x[(int64_t)xr * n + 4 * q + c] : 0.0f;
        }
        float om[4];
        if (a.eps) {
#pragma unroll
            for (int c = 0; c < 4; ++c) om[c] = live[c] ? a.eps[off + c] : 0.0f;
        } else {
            uint32_t r[4];
            abc_philox(a.j0 + (uint32_t)s, t, a.i0 + (uint32_t)i, (uint32_t)q, a.k0, a.k1, r);
            abc_pair(r[0], r[1], om[0], om[1]);
            abc_pair(r[2], r[3], om[2], om[3]);
        }
        float part = w[0] * xv[0];
        part = fmaf(w[1], xv[1], part);
        part = fmaf(w[2], xv[2], part);
        part = fmaf(w[3], xv[3], part);
        const float y = hebb_group_sum<G>(part);
        const float ay = __fmul_rn(alpha, y);
        const float by2 = __fmul_rn(beta, __fmul_rn(y, y));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float dw = __fsub_rn(__fmul_rn(ay, __fsub_rn(xv[c], theta)), __fmul_rn(by2, w[c]));
            float v = __fadd_rn(__fadd_rn(w[c], dw), __fmul_rn(a.sigma, om[c]));
            v = v < nb ? nb : v;
            v = v > b ? b : v;
            w[c] = live[c] ? v : 0.0f;
        }
        if (a.traj) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (live[c]) a.traj[off + c] = w[c];
        }
        off += row_step;
        xr = xr + 1 == a.N_x ? 0 : xr + 1;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (live[c]) a.w[i * n + 4 * q + c] = w[c];
}

__global__ __launch_bounds__(256) void hebb_noise_kernel(float* __restrict__ omega, const int64_t* t_dev, uint32_t k0,
                                                         uint32_t k1, uint32_t t, uint32_t i0, int64_t n_i, uint32_t j0,
                                                         int64_t n_j, int n) {
    const int nb = (n + 3) / 4;
    const int64_t total = n_i * n_j * nb;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    if (t_dev) t = (uint32_t)*t_dev;
    const int b = (int)(idx % nb);
    const int64_t row = idx / nb;  // c * n_i + a
    const int64_t c = row / n_i, i = row - c * n_i;
    uint32_t w[4];
    abc_philox(j0 + (uint32_t)c, t, i0 + (uint32_t)i, (uint32_t)b, k0, k1, w);
    float v[4];
    abc_pair(w[0], w[1], v[0], v[1]);
    abc_pair(w[2], w[3], v[2], v[3]);
    float* out = omega + row * n;
    for (int p = 0; p < 4; ++p)
        if (4 * b + p < n) out[4 * b + p] = v[p];
}

// the group width of n neurons: ceil(n / 4) rounded up to a power of two, as log2 (0 .. 4)
static int hebb_log2_group(int n) {
    const int blocks = (n + 3) / 4;
    int lg = 0;
    while ((1 << lg) < blocks) ++lg;
    return lg;
}

static int hebb_check_stream(const char* fn, int64_t t, int64_t i0, int64_t n_i, int64_t j0, int64_t n_j) {
    if (t < 0 || t > 0x7fffffffLL || i0 < 0 || n_i < 0 || j0 < 0 || n_j < 0 || i0 > (1LL << 31) || n_i > (1LL << 31) ||
        i0 + n_i > (1LL << 31) || j0 > 0x7fffffffLL || n_j > 0x7fffffffLL || j0 + n_j > 0x7fffffffLL)
        return fail(TNF_EINVAL, "%s: t=%lld i0=%lld n_i=%lld j0=%lld n_j=%lld outside the stream's counters", fn, (long long)t,
                    (long long)i0, (long long)n_i, (long long)j0, (long long)n_j);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_hebb_supported(int32_t n) { return n >= 1 && n <= TNF_HEBB_MAX_N ? 1 : 0; }

int64_t tnf_hebb_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_HEBB_COUNTERS) return fail(TNF_EINVAL, "tnf_hebb_launch_count: counter %d", which);
    return g_hebb_launches[which].load(std::memory_order_relaxed);
}

int tnf_hebb_simulate_f32(const float* z, const float* x, const float* w0, const float* eps, float* w, float* traj,
                          const int64_t* t_dev, int64_t seed, int64_t t, int64_t i0, int64_t N, int64_t N_w0, int32_t n,
                          int32_t N_x, int64_t j0, int64_t n_steps, float sigma_eps, void* stream) {
    const char* fn = "tnf_hebb_simulate_f32";
    if (!tnf_hebb_supported(n))
        return fail(TNF_EUNSUPPORTED, "%s: n=%d, the kernel exists for 1 <= n <= %d", fn, n, TNF_HEBB_MAX_N);
    if (!z || !x || !w0 || !w) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (int rc = hebb_check_stream(fn, t, i0, N, j0, n_steps)) return rc;
    if (N_w0 != 1 && N_w0 != N) return fail(TNF_EINVAL, "%s: N_w0=%lld must be 1 or N=%lld", fn, (long long)N_w0, (long long)N);
    if (N_x < 1) return fail(TNF_EINVAL, "%s: N_x=%d, must be at least 1", fn, N_x);
    if (!(sigma_eps >= 0.0f)) return fail(TNF_EINVAL, "%s: sigma_eps=%g, must be >= 0", fn, (double)sigma_eps);
    if (N == 0 || n_steps == 0) return TNF_OK;
    const int lg = hebb_log2_group(n);
    const int G = 1 << lg;
    // a few hundred simulations are a latency problem: one wave per workgroup spreads them over the CUs
    const int block = N * G <= 64 * 1024 ? 64 : 256;
    const int64_t blocks = (N * G + block - 1) / block;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
    const size_t smem = (size_t)N_x * 4 * G * sizeof(float);
    const bool ldsx = smem <= 64 * 1024;
    const HebbArgs a{z, x, w0, eps, w, traj, t_dev, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32),
                     (uint32_t)t, (uint32_t)i0, (uint32_t)j0, N, n_steps, N_w0 == 1 ? 0 : n, n, N_x, sigma_eps};
    const int rc = dispatch_range<0, 4>(lg, [&](auto lgc) {
        return dispatch_bool(ldsx, [&](auto lc) {
            constexpr int Gc = 1 << decltype(lgc)::value;
            constexpr bool L = decltype(lc)::value;
            return launch_lds(fn, hebb_sim_kernel<Gc, L>, dim3((unsigned)blocks), dim3(block), L ? smem : 0, as_stream(stream),
                              a);
        });
    });
    if (rc) return rc;
    hebb_count(TNF_HEBB_COUNT_SIM);
    return check_launch(fn);
}

int tnf_hebb_noise_f32(float* omega, const int64_t* t_dev, int64_t seed, int64_t t, int64_t i0, int64_t n_i, int64_t j0,
                       int64_t n_j, int32_t n, void* stream) {
    const char* fn = "tnf_hebb_noise_f32";
    if (!tnf_hebb_supported(n))
        return fail(TNF_EUNSUPPORTED, "%s: n=%d, the stream serves 1 <= n <= %d", fn, n, TNF_HEBB_MAX_N);
    if (int rc = hebb_check_stream(fn, t, i0, n_i, j0, n_j)) return rc;
    if (!omega) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (n_i == 0 || n_j == 0) return TNF_OK;
    const int nb = (n + 3) / 4;
    if (n_i > 0x7fffffffffffLL / n_j / nb) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
    const int64_t blocks = (n_i * n_j * nb + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "%s: grid too large", fn);
    hipLaunchKernelGGL(hebb_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), omega, t_dev,
                       (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), (uint32_t)t, (uint32_t)i0, n_i,
                       (uint32_t)j0, n_j, (int)n);
    hebb_count(TNF_HEBB_COUNT_NOISE);
    return check_launch(fn);
}

}  // extern "C"
