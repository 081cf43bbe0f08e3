// The backward of log_prob for per-context coupling flows with 17 <= U <= 64 hidden units and few samples per context
// (include/tnf_ctxwide.h): one parameter row per context m, 1 <= N <= 31 rows per context, the whole reversible backward
// in ONE launch at every 2 <= D <= 64.  The forward half is tnf_ctx_wide_log_prob_f32 (flow_ctx_wide.hip), which keeps z0.
//
// The slice and the walk through a coupling layer are ctx_bwd_walk.h's, as in flow_ctx_bwd.hip: ctx_bwd_coupling<true,
// STEP> with one workgroup of 4, 8 or 16 waves per context (cwb_waves) (a slice is 20 .. 150 KB here, so one context per workgroup is
// all that fits, and a layer has 2 N U >= 34 N items per step for its lanes).  A context's gradient is a contraction
// over <= 31 samples that is written once: nothing is accumulated across tiles or workgroups, which is why this layout,
// unlike many samples per row (coupling_wide_bwd.hip), needs neither records in HBM nor atomics.  Every output element
// is computed by one lane in full, in a fixed order: the results do not depend on the team size.
//
// The layer's STEP and the BatchNorm / Affine map between layers are copies of CtxTrainStep and ctxt_between of
// flow_ctx_bwd.hip: that file defines extern "C" entries and cannot be included, and moving the two into
// ctx_bwd_walk.h would have to leave flow_ctx_bwd.hip's machine code unchanged to be allowed.  The kernel differs from
// ctx_train_bwd_kernel<true> in its team size and its launch (dynamic LDS above 64 KB) only.
#include "ctx_wide.h"
#include "../../include/tnf_ctxwide.h"

namespace tnf {

constexpr int CWB_MAX_WAVES = 16;  // the team is the launch's block: 4, 8 or 16 waves, all on one context

// the team size of a shape: cwb_waves (ctx_wide.h)

extern std::atomic<long long> g_ctxwide_launches[TNF_CTXWIDE_COUNTERS];  // flow_ctx_wide.hip

struct CtxWideBwdArgs {
    const float* z0;       // (M, N, D)
    const float* params;   // (M, pstride)
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    const float* g_lp;     // (M, N)
    float* g_params;       // (M, gpstride)
    float* g_z;            // (M, N, D) or NULL
    int64_t M, pstride, gpstride;
    int N, D, S, L, U;
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

// The coupling layer itself (ctx_bwd_coupling's STEP).  log_prob ran z2 = (y2 - t) e^-s; with G the gradient at
// (z1, z2) and gl at sum(s):  rebuild y2 = t + z2 e^s;  G(y2) = G2 e^-s;  d t = -G2 e^-s;  d s = gl - G2 z2
struct CtxWideStep {
    static __device__ __forceinline__ void apply(float* zs, float* gs, const float* gl, float* ts, int ND, int i, int at,
                                                 int n) {
        const float tv = ts[i], s = ts[ND + i];
        const float z2 = zs[at], G2 = gs[at];
        const float gy = G2 * expf(-s);
        zs[at] = __builtin_fmaf(z2, expf(s), tv);
        gs[at] = gy;
        ts[i] = -gy;
        ts[ND + i] = __builtin_fmaf(-G2, z2, gl[n]);
    }
};

// The parameter-free BatchNorm layer c and, behind the lower layer, the stage's Affine block, as the walk passes them:
//   BatchNorm (frozen): log_prob ran x = y alpha + mu, so y = (x - mu) / alpha and G(y) = G(x) alpha
//   Affine:             log_prob ran x = (y - shift) e^-a, so y = x e^a + shift, G(y) = G(x) e^-a,
//                       d shift = -sum_n G(y), d a = sum_n (gl - G(x) x)
// ap / ga: the Affine block [a (D) | shift (D)] in LDS and its gradient slots, or NULL.  One lane per feature: the sums
// over the samples are sequential.
__device__ __forceinline__ void ctxw_between(const float* __restrict__ mean, const float* __restrict__ alpha, const float* ap,
                                             float* __restrict__ ga, float* zs, float* gs, const float* gl, int N, int D,
                                             int t, int nt) {
    for (int d = t; d < D; d += nt) {
        const float mu = mean[d], al = alpha[d];
        float a = 0.f, sh = 0.f, ea = 1.f, ema = 1.f;
        if (ap) {
            a = ap[d];
            sh = ap[D + d];
            ea = expf(a);
            ema = expf(-a);
        }
        float da = 0.f, dsh = 0.f;
        for (int n = 0; n < N; ++n) {
            float x = zs[n * D + d], G = gs[n * D + d];
            x = (x - mu) / al;
            G *= al;
            if (ap) {
                da += __builtin_fmaf(-G, x, gl[n]);
                G *= ema;
                dsh -= G;
                x = __builtin_fmaf(x, ea, sh);
            }
            zs[n * D + d] = x;
            gs[n * D + d] = G;
        }
        if (ap) {
            ga[d] = da;
            ga[D + d] = dsh;
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(CWB_MAX_WAVES * 64) ctx_wide_bwd_kernel(CtxWideBwdArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float cwb_lds[];
    const int t = threadIdx.x, nt = blockDim.x;
    const int64_t m = grid_m();
    if (m >= a.M) return;  // the whole workgroup leaves
    const int N = a.N, D = a.D, L = a.L, U = a.U, h = D / 2, hh = D - h;
    const FlowLayout fl = flow_layout(D, a.S, L, U);
    const int n_up = (int)fl.p_up, n_low = (int)fl.p_low + 2 * D;
    const int n_wb = n_up > n_low ? n_up : n_low;

    // the slice of ctx_bwd_walk.h
    float* zs = cwb_lds;
    float* gs = zs + N * D;
    float* gl = gs + N * D;
    float* wb = gl + N;
    float* act = wb + n_wb;
    float* ts = act + 2 * L * N * U;

    const float* p = a.params + m * a.pstride;
    float* gp = a.g_params + m * a.gpstride;
    {
        const float* z0 = a.z0 + m * (int64_t)N * D;
        const float* glp = a.g_lp + m * (int64_t)N;
        for (int i = t; i < N * D; i += nt) {
            const float v = z0[i];
            zs[i] = v;
            gs[i] = -glp[i / D] * v;  // d(-|z0|^2 / 2) / d z0, times the upstream gradient
        }
        for (int n = t; n < N; n += nt) gl[n] = -glp[n];  // log_prob subtracts the summed log-det
    }
    __syncthreads();

    for (int st = 0; st < a.S; ++st) {
        const float* ps = p + st * fl.stage;
        float* gst = gp + st * fl.stage;
        const int c0 = 2 * st, c1 = 2 * st + 1;
        // the upper layer: conditioner = the first h features, transformed = the other D - h
        for (int i = t; i < n_up; i += nt) wb[i] = ps[i];
        __syncthreads();
        ctx_bwd_coupling<true, CtxWideStep>(wb, gst, zs, gs, gl, act, ts, N, D, L, U, h, hh, 0, h, t, nt);
        ctxw_between(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, nullptr, nullptr, zs, gs, gl, N, D, t, nt);
        // the lower layer with the Affine block behind it: conditioner = the last D - h features
        for (int i = t; i < n_low; i += nt) wb[i] = ps[fl.p_up + i];
        __syncthreads();
        ctx_bwd_coupling<true, CtxWideStep>(wb, gst + fl.p_up, zs, gs, gl, act, ts, N, D, L, U, hh, h, h, 0, t, nt);
        ctxw_between(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, wb + fl.p_low, gst + fl.p_up + fl.p_low, zs, gs, gl, N, D, t,
                     nt);
    }

    if (a.g_z) {
        float* gz = a.g_z + m * (int64_t)N * D;
        for (int i = t; i < N * D; i += nt) gz[i] = gs[i];
    }
}

// the checks of ctx_bwd_check (ctx_bwd_walk.h), in its order, with this family's predicate and grid
static int ctxwide_bwd_check(const char* fn, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U,
                             int64_t pstride, int64_t gpstride) {
    if (M < 1 || N < 0) return fail(TNF_EINVAL, "%s: M=%lld N=%lld", fn, (long long)M, (long long)N);
    if (M > (int64_t)32768 * 65535) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!ctx_wide_train_supported(D, S, L, U, N == 0 ? 1 : N))
        return fail(TNF_EUNSUPPORTED, "%s: no wide per-context backward for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L, U,
                    (long long)N);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    if (gpstride < need)
        return fail(TNF_EINVAL, "%s: gradient row has %lld elements, flow needs %lld", fn, (long long)gpstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_wide_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                  const float* g_lp, float* g_params, float* g_z, int64_t M, int64_t N, int32_t D,
                                  int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_ctx_wide_log_prob_bwd_f32";
    if (!z0 || !params || !bn_mean || !bn_alpha || !g_lp || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (const int rc = ctxwide_bwd_check(fn, M, N, D, S, L, U, pstride, gpstride)) return rc;
    if (g_z == z0) return fail(TNF_EINVAL, "%s: g_z must not alias z0", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (N == 0) return TNF_OK;
    const CtxWideBwdArgs a{z0, params, bn_mean, bn_alpha, g_lp, g_params, g_z, M, pstride, gpstride, (int)N, D, S, L, U,
                           g_launch_gate};
    const size_t smem = (size_t)ctx_wide_lds_bytes(1, D, S, L, U, N);
    g_ctxwide_launches[TNF_CTXWIDE_COUNT_LOG_PROB_BWD].fetch_add(1, std::memory_order_relaxed);
    if (const int rc = launch_lds("ctx_wide_bwd", ctx_wide_bwd_kernel, grid_xm(1, M), dim3(cwb_waves((int)N, D, U) * 64), smem,
                                  as_stream(stream), a))
        return rc;
    return check_launch("ctx_wide_bwd");
}

}  // extern "C"
