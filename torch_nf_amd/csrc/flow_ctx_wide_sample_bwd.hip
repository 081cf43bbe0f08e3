// The backward of frozen-statistics sampling for per-context coupling flows with 17 <= U <= 64 hidden units and few
// samples per context (include/tnf_ctxwidesample.h): one parameter row per context m, 1 <= N <= 31 draws per context, the
// whole reversible backward in ONE launch at every 2 <= D <= 64.  The forward half is tnf_ctx_wide_forward_f32
// (flow_ctx_wide.hip), whose output z is all this kernel needs of it.
//
// The walk is ctx_sample_bwd_kernel<true>'s (flow_ctx_sample_bwd.hip) -- stages last to first; per stage the Affine block,
// BatchNorm c1, the lower coupling layer, BatchNorm c0, the upper coupling layer; each layer's input rebuilt from z by
// the inverse map -- with the step and the between-layers map of ctx_sample_step.h and the coupling walk of
// ctx_bwd_walk.h.  The mapping is ctx_wide_bwd_kernel's (flow_ctx_wide_bwd.hip): one workgroup per context, the context's
// slice (20 .. 150 KB) as dynamic LDS.  Every output element is computed by one lane in full, in a fixed order: the
// results do not depend on the team size.
//
// Team size.  The kernel is instantiated for teams of 4, 8 and 16 waves, each with its own launch bounds, so a small
// team is not held to the register cap of a 1,024-thread block and the team's lane count is a compile-time stride.  The
// automatic choice is cws_waves below; tnf_ctx_wide_sample_set_waves overrides it process-wide so that one build can
// time and compare the three (tools/ctxwidesamplebench.py).
#include "ctx_sample_step.h"
#include "ctx_wide.h"
#include "../../include/tnf_ctxwidesample.h"

namespace tnf {

static std::atomic<long long> g_ctxwidesample_launches;
static std::atomic<int> g_ctxwidesample_waves{0};  // 0: automatic; 4, 8, 16: forced (tnf_ctx_wide_sample_set_waves)

// The automatic team size of a shape, from the three instantiations timed in one build (DESIGN.md 26.6, table 2 of
// profiles/r23_ctxwidesamplebench_first_rule.txt, where the automatic team was still cwb_waves, and of
// profiles/r23_ctxwidesamplebench.txt, this rule's run, where it is the fastest team in all 30 cells; M N = 2^16, S = 2, L = 2).  It is cwb_waves (ctx_wide.h), the rule of the
// log_prob direction, whose walk has the same steps with the same item counts -- the fastest team in 25 of the 30 cells
// -- with two departures, both towards four waves where a context has few samples:
//   * up to 8 samples and 2 U U <= 1,024 (U <= 22): only the first and last layer's contractions are wide (D = 64), and
//     four waves are 1.27 x (N = 1) and 1.11 x (N = 8) faster than cwb_waves' eight at (D = 64, U = 20); at N = 31 eight
//     win 1.29 x and stay.
//   * one sample, more than 48 units and D <= 8: at U = 64 four waves are 1.03 .. 1.05 x faster than eight (spreads
//     <= 0.2 %); at D = 32 and 64 eight win 1.09 .. 1.15 x and stay.  The departure is drawn at the tile class of the
//     measured U = 64 (49 .. 64 units); 23 .. 48 units at one sample were not measured and keep cwb_waves' team.
// Each departure rests on one end of a range: the first on D = 64 alone (at smaller D cwb_waves gives four waves to these
// units anyway, so it acts only from D = 52 on), the second on U = 64 alone.  Not measured: U between 21 and 63, N
// between 2 and 7 and between 9 and 30, D between 9 and 31.  The results are the same bits for every team size.
inline int cws_waves(int N, int D, int U) {
    if (N <= 8 && 2 * U * U <= 1024) return 4;
    if (N == 1 && U > 48 && D <= 8) return 4;
    return cwb_waves(N, D, U);
}

struct CtxWideSampleArgs {
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
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

template <int WAVES>
__global__ void __launch_bounds__(WAVES * 64) ctx_wide_sample_bwd_kernel(CtxWideSampleArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float cws_lds[];
    constexpr int nt = WAVES * 64;
    const int t = threadIdx.x;
    const int64_t m = grid_m();
    if (m >= a.M) return;  // the whole workgroup leaves
    const int N = a.N, D = a.D, L = a.L, U = a.U, h = D / 2, hh = D - h;
    const FlowLayout fl = flow_layout(D, a.S, L, U);
    const int n_up = (int)fl.p_up, n_low = (int)fl.p_low + 2 * D;
    const int n_wb = n_up > n_low ? n_up : n_low;

    // the slice of ctx_bwd_walk.h
    float* zs = cws_lds;
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
    __syncthreads();

    for (int st = a.S - 1; st >= 0; --st) {
        const float* ps = p + st * fl.stage;
        float* gst = gp + st * fl.stage;
        const int c0 = 2 * st, c1 = 2 * st + 1;
        // the Affine block and BatchNorm c1, then the lower layer in front of them: conditioner = the last D - h features
        for (int i = t; i < n_low; i += nt) wb[i] = ps[fl.p_up + i];
        __syncthreads();
        ctxs_between<true>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, wb + fl.p_low, gst + fl.p_up + fl.p_low, zs, gs, gl, N, D,
                           t, nt);
        ctx_bwd_coupling<true, CtxSampleStep>(wb, gst + fl.p_up, zs, gs, gl, act, ts, N, D, L, U, hh, h, h, 0, t, nt);
        // BatchNorm c0, then the upper layer: conditioner = the first h features, transformed = the other D - h.  The
        // lower layer's last barrier separates its reads of wb from these writes; ctxs_between's separates the writes
        // from the upper layer's reads (BatchNorm reads no parameter)
        for (int i = t; i < n_up; i += nt) wb[i] = ps[i];
        ctxs_between<true>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, nullptr, nullptr, zs, gs, gl, N, D, t, nt);
        ctx_bwd_coupling<true, CtxSampleStep>(wb, gst, zs, gs, gl, act, ts, N, D, L, U, h, hh, 0, h, t, nt);
    }

    if (a.g_omega) {
        float* go = a.g_omega + m * (int64_t)N * D;
        for (int i = t; i < N * D; i += nt) go[i] = gs[i];
    }
}

// the checks of ctx_bwd_check (ctx_bwd_walk.h), in its order, with this family's predicate and grid
static int ctxwidesample_check(const char* fn, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U,
                               int64_t pstride, int64_t gpstride) {
    if (M < 1 || N < 0) return fail(TNF_EINVAL, "%s: M=%lld N=%lld", fn, (long long)M, (long long)N);
    if (M > (int64_t)32768 * 65535) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    const int64_t n1 = N == 0 ? 1 : N;
    if (!(ctx_wide_supported(D, S, L, U, n1) && ctx_wide_train_supported(D, S, L, U, n1)))
        return fail(TNF_EUNSUPPORTED, "%s: no wide per-context sampling backward for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L,
                    U, (long long)N);
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

int tnf_ctx_wide_sample_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return ctx_wide_supported(D, S, L, U, N) && ctx_wide_train_supported(D, S, L, U, N) ? 1 : 0;
}

int64_t tnf_ctx_wide_sample_launch_count(void) { return g_ctxwidesample_launches.load(std::memory_order_relaxed); }

int tnf_ctx_wide_sample_waves(int32_t D, int32_t U, int64_t N) {
    return ctx_wide_domain(D, 1, U, N) ? cws_waves((int)N, D, U) : -1;
}

int tnf_ctx_wide_sample_set_waves(int32_t waves) {
    if (waves != 0 && waves != 4 && waves != 8 && waves != 16)
        return fail(TNF_EINVAL, "tnf_ctx_wide_sample_set_waves: waves=%d is not 0 (automatic), 4, 8 or 16", waves);
    return g_ctxwidesample_waves.exchange(waves, std::memory_order_relaxed);
}

int tnf_ctx_wide_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                                const float* g_z, const float* g_sld, float* g_params, float* g_omega, int64_t M, int64_t N,
                                int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_ctx_wide_sample_bwd_f32";
    if (!z || !params || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: no upstream gradient (g_z and g_sld both NULL)", fn);
    if (const int rc = ctxwidesample_check(fn, M, N, D, S, L, U, pstride, gpstride)) return rc;
    if (g_omega && (g_omega == z || g_omega == g_z)) return fail(TNF_EINVAL, "%s: g_omega must not alias z or g_z", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (N == 0) return TNF_OK;
    const CtxWideSampleArgs a{z, params, bn_mean, bn_alpha, g_z, g_sld, g_params, g_omega, M, pstride, gpstride,
                              (int)N, D, S, L, U, g_launch_gate};
    const size_t smem = (size_t)ctx_wide_lds_bytes(1, D, S, L, U, N);
    const int forced = g_ctxwidesample_waves.load(std::memory_order_relaxed);
    const int waves = forced ? forced : cws_waves((int)N, D, U);
    const dim3 grid = grid_xm(1, M), block(waves * 64);
    const hipStream_t st = as_stream(stream);
    int rc;
    if (waves == 4)
        rc = launch_lds("ctx_wide_sample_bwd", ctx_wide_sample_bwd_kernel<4>, grid, block, smem, st, a);
    else if (waves == 8)
        rc = launch_lds("ctx_wide_sample_bwd", ctx_wide_sample_bwd_kernel<8>, grid, block, smem, st, a);
    else
        rc = launch_lds("ctx_wide_sample_bwd", ctx_wide_sample_bwd_kernel<16>, grid, block, smem, st, a);
    if (rc) return rc;
    g_ctxwidesample_launches.fetch_add(1, std::memory_order_relaxed);  // the call reached its launch
    return check_launch("ctx_wide_sample_bwd");
}

}  // extern "C"
