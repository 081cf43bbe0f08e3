// The backward of log_prob for per-context coupling flows with few samples per context (include/tnf_ctxtrain.h): one
// parameter row per context m, 1 <= N <= 31 rows per context, the whole reversible backward in ONE launch at every
// 2 <= D <= 64.  The forward half is tnf_ctx_flow_log_prob_f32 (flow_ctx.hip), which keeps z0.
//
// The mapping, the slice and the walk through a coupling layer are ctx_bwd_walk.h's, shared with the backward of
// sampling.  In this direction a context's slice holds
//   zs (N, D)          z0 on entry, the input z of log_prob at the end
//   gs (N, D)          -g_lp z0 on entry, g_z at the end
//   gl (N)             -g_lp
// and the walk visits the bijectors first to last -- the reverse of the order log_prob evaluated them in.  At a coupling
// layer it recomputes the twin nets from the conditioner half, rebuilds the layer's input z2 <- t + z2 e^s (the
// sampling-direction map), sends the deltas back through the transposed weights, contracts activations with deltas over
// the context's samples and writes each weight and bias gradient once, at the slot the parameter has in the row.
// BatchNorm maps are constants (the shared (2S, D) statistics); the Affine block's alpha / shift gradients, the log-det
// term of alpha included, are written the same way.
#include "ctx_bwd_walk.h"
#include "../../include/tnf_ctxtrain.h"

namespace tnf {

static std::atomic<long long> g_ctxtrain_launches;

struct CtxTrainArgs {
    const float* z0;       // (M, N, D)
    const float* params;   // (M, pstride)
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    const float* g_lp;     // (M, N)
    float* g_params;       // (M, gpstride)
    float* g_z;            // (M, N, D) or NULL
    int64_t M, pstride, gpstride;
    int N, D, S, L, U;
    int slice;             // floats of one context's LDS slice
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

// The coupling layer itself (ctx_bwd_coupling's STEP).  log_prob ran z2 = (y2 - t) e^-s; with G the gradient at
// (z1, z2) and gl at sum(s):  rebuild y2 = t + z2 e^s;  G(y2) = G2 e^-s;  d t = -G2 e^-s;  d s = gl - G2 z2
struct CtxTrainStep {
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
template <bool TEAM>
__device__ __forceinline__ void ctxt_between(const float* __restrict__ mean, const float* __restrict__ alpha, const float* ap,
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
    ctx_bwd_sync<TEAM>();
}

template <bool TEAM>
__global__ void __launch_bounds__(CTX_BWD_WAVES * 64) ctx_train_bwd_kernel(CtxTrainArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float ctxt_lds[];
    // TEAM: the workgroup's CTX_BWD_WAVES waves serve one context together; else one wave per context
    const int wave = TEAM ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = TEAM ? threadIdx.x : threadIdx.x & 63, nt = TEAM ? CTX_BWD_WAVES * 64 : 64;
    const int64_t m = TEAM ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (m >= a.M) return;  // whole waves leave: without TEAM nothing below synchronises across waves
    const int N = a.N, D = a.D, L = a.L, U = a.U, h = D / 2, hh = D - h;
    const FlowLayout fl = flow_layout(D, a.S, L, U);
    const int n_up = (int)fl.p_up, n_low = (int)fl.p_low + 2 * D;
    const int n_wb = n_up > n_low ? n_up : n_low;

    float* zs = ctxt_lds + (int64_t)wave * a.slice;
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
    ctx_bwd_sync<TEAM>();

    for (int st = 0; st < a.S; ++st) {
        const float* ps = p + st * fl.stage;
        float* gst = gp + st * fl.stage;
        const int c0 = 2 * st, c1 = 2 * st + 1;
        // the upper layer: conditioner = the first h features, transformed = the other D - h
        for (int i = t; i < n_up; i += nt) wb[i] = ps[i];
        ctx_bwd_sync<TEAM>();
        ctx_bwd_coupling<TEAM, CtxTrainStep>(wb, gst, zs, gs, gl, act, ts, N, D, L, U, h, hh, 0, h, t, nt);
        ctxt_between<TEAM>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, nullptr, nullptr, zs, gs, gl, N, D, t, nt);
        // the lower layer with the Affine block behind it: conditioner = the last D - h features
        for (int i = t; i < n_low; i += nt) wb[i] = ps[fl.p_up + i];
        ctx_bwd_sync<TEAM>();
        ctx_bwd_coupling<TEAM, CtxTrainStep>(wb, gst + fl.p_up, zs, gs, gl, act, ts, N, D, L, U, hh, h, h, 0, t, nt);
        ctxt_between<TEAM>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, wb + fl.p_low, gst + fl.p_up + fl.p_low, zs, gs, gl, N, D,
                           t, nt);
    }

    if (a.g_z) {
        float* gz = a.g_z + m * (int64_t)N * D;
        for (int i = t; i < N * D; i += nt) gz[i] = gs[i];
    }
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_train_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) { return ctx_bwd_supported(D, S, L, U, N); }

int64_t tnf_ctx_train_launch_count(void) { return g_ctxtrain_launches.load(std::memory_order_relaxed); }

int tnf_ctx_train_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                   const float* g_lp, float* g_params, float* g_z, int64_t M, int64_t N, int32_t D,
                                   int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_ctx_train_log_prob_bwd_f32";
    if (!z0 || !params || !bn_mean || !bn_alpha || !g_lp || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (const int rc = ctx_bwd_check(fn, M, N, D, S, L, U, pstride, gpstride)) return rc;
    if (g_z == z0) return fail(TNF_EINVAL, "%s: g_z must not alias z0", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (N == 0) return TNF_OK;
    const CtxTrainArgs a{z0, params, bn_mean, bn_alpha, g_lp, g_params, g_z, M, pstride, gpstride, (int)N, D, S, L, U,
                         0 /* slice: ctx_bwd_launch */, g_launch_gate};
    return ctx_bwd_launch(fn, "ctx_train_bwd", ctx_train_bwd_kernel<false>, ctx_train_bwd_kernel<true>, a,
                          g_ctxtrain_launches, stream);
}

}  // extern "C"
