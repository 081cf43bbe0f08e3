// The backward of frozen-statistics sampling for per-context coupling flows with few samples per context
// (include/tnf_ctxsample.h): one parameter row per context m, 1 <= N <= 31 draws per context, the whole reversible
// backward in ONE launch at every 2 <= D <= 64.  The forward half is tnf_ctx_flow_forward_f32 (flow_ctx.hip), whose
// output z is all this kernel needs of it.
//
// The mapping, the slice and the walk through a coupling layer are ctx_bwd_walk.h's, shared with the backward of
// log_prob.  In this direction a context's slice holds
//   zs (N, D)          the forward's output z on entry, the draw omega at the end
//   gs (N, D)          g_z on entry (0 where it is NULL), g_omega at the end
//   gl (N)             g_sld (0 where it is NULL)
// and the walk visits the bijectors last to first -- the reverse of the order the sampling pass evaluated them in.  Each
// stage is undone as: the Affine block, BatchNorm c1, the lower coupling layer, BatchNorm c0, the upper coupling layer.
// At a coupling layer it recomputes the twin nets from the conditioner half (which the layer leaves unchanged), rebuilds
// the layer's input x2 <- (y2 - t) e^-s (the inverse map), sends the deltas back through the transposed weights,
// contracts activations with deltas over the context's samples and writes each weight and bias gradient once, at the
// slot the parameter has in the row.  BatchNorm maps are constants (the shared (2S, D) statistics: no gradient).
// The layer's STEP and the map between layers are ctx_sample_step.h's, shared with flow_ctx_wide_sample_bwd.hip.
#include "ctx_sample_step.h"
#include "../../include/tnf_ctxsample.h"

namespace tnf {

static std::atomic<long long> g_ctxsample_launches;

struct CtxSampleArgs {
    const float* z;        // (M, N, D): the forward's output
    const float* params;   // (M, pstride)
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    const float* g_z;      // (M, N, D) or NULL (zero)
    const float* g_sld;    // (M, N) or NULL (zero)
    float* g_params;       // (M, gpstride)
    float* g_omega;        // (M, N, D) or NULL
    int64_t M, pstride, gpstride;
    int N, D, S, L, U;
    int slice;             // floats of one context's LDS slice
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

template <bool TEAM>
__global__ void __launch_bounds__(CTX_BWD_WAVES * 64) ctx_sample_bwd_kernel(CtxSampleArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float ctxs_lds[];
    // TEAM: the workgroup's CTX_BWD_WAVES waves serve one context together; else one wave per context
    const int wave = TEAM ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = TEAM ? threadIdx.x : threadIdx.x & 63, nt = TEAM ? CTX_BWD_WAVES * 64 : 64;
    const int64_t m = TEAM ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (m >= a.M) return;  // whole waves leave: without TEAM nothing below synchronises across waves
    const int N = a.N, D = a.D, L = a.L, U = a.U, h = D / 2, hh = D - h;
    const FlowLayout fl = flow_layout(D, a.S, L, U);
    const int n_up = (int)fl.p_up, n_low = (int)fl.p_low + 2 * D;
    const int n_wb = n_up > n_low ? n_up : n_low;

    float* zs = ctxs_lds + (int64_t)wave * a.slice;
    float* gs = zs + N * D;
    float* gl = gs + N * D;
    float* wb = gl + N;
    float* act = wb + n_wb;
    float* ts = act + 2 * L * N * U;

    const float* p = a.params + m * a.pstride;
    float* gp = a.g_params + m * a.gpstride;
    {
        const float* z = a.z + m * (int64_t)N * D;
        const float* gz = a.g_z ? a.g_z + m * (int64_t)N * D : nullptr;
        const float* gsld = a.g_sld ? a.g_sld + m * (int64_t)N : nullptr;
        for (int i = t; i < N * D; i += nt) {
            zs[i] = z[i];
            gs[i] = gz ? gz[i] : 0.f;
        }
        for (int n = t; n < N; n += nt) gl[n] = gsld ? gsld[n] : 0.f;
    }
    ctx_bwd_sync<TEAM>();

    for (int st = a.S - 1; st >= 0; --st) {
        const float* ps = p + st * fl.stage;
        float* gst = gp + st * fl.stage;
        const int c0 = 2 * st, c1 = 2 * st + 1;
        // the Affine block and BatchNorm c1, then the lower layer in front of them: conditioner = the last D - h features
        for (int i = t; i < n_low; i += nt) wb[i] = ps[fl.p_up + i];
        ctx_bwd_sync<TEAM>();
        ctxs_between<TEAM>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, wb + fl.p_low, gst + fl.p_up + fl.p_low, zs, gs, gl, N, D,
                           t, nt);
        ctx_bwd_coupling<TEAM, CtxSampleStep>(wb, gst + fl.p_up, zs, gs, gl, act, ts, N, D, L, U, hh, h, h, 0, t, nt);
        // BatchNorm c0, then the upper layer: conditioner = the first h features, transformed = the other D - h
        for (int i = t; i < n_up; i += nt) wb[i] = ps[i];
        ctxs_between<TEAM>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, nullptr, nullptr, zs, gs, gl, N, D, t, nt);
        ctx_bwd_coupling<TEAM, CtxSampleStep>(wb, gst, zs, gs, gl, act, ts, N, D, L, U, h, hh, 0, h, t, nt);
    }

    if (a.g_omega) {
        float* go = a.g_omega + m * (int64_t)N * D;
        for (int i = t; i < N * D; i += nt) go[i] = gs[i];
    }
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_sample_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) { return ctx_bwd_supported(D, S, L, U, N); }

int64_t tnf_ctx_sample_launch_count(void) { return g_ctxsample_launches.load(std::memory_order_relaxed); }

int tnf_ctx_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha, const float* g_z,
                           const float* g_sld, float* g_params, float* g_omega, int64_t M, int64_t N, int32_t D, int32_t S,
                           int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_ctx_sample_bwd_f32";
    if (!z || !params || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: no upstream gradient (g_z and g_sld both NULL)", fn);
    if (const int rc = ctx_bwd_check(fn, M, N, D, S, L, U, pstride, gpstride)) return rc;
    if (g_omega && (g_omega == z || g_omega == g_z)) return fail(TNF_EINVAL, "%s: g_omega must not alias z or g_z", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (N == 0) return TNF_OK;
    const CtxSampleArgs a{z, params, bn_mean, bn_alpha, g_z, g_sld, g_params, g_omega, M, pstride, gpstride, (int)N, D, S, L, U,
                          0 /* slice: ctx_bwd_launch */, g_launch_gate};
    return ctx_bwd_launch(fn, "ctx_sample_bwd", ctx_sample_bwd_kernel<false>, ctx_sample_bwd_kernel<true>, a,
                          g_ctxsample_launches, stream);
}

}  // extern "C"
