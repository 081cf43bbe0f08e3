// The backward of frozen-statistics sampling for per-context coupling flows with few samples per context
// (include/tnf_ctxsample.h): one parameter row per context m, 1 <= N <= 31 draws per context, the whole reversible
// backward in ONE launch at every 2 <= D <= 64.  The forward half is tnf_ctx_flow_forward_f32 (flow_ctx.hip), whose
// output z is all this kernel needs of it.
//
// The mirror image of flow_ctx_bwd.hip: the same mapping, the same slice, the same arithmetic, the other direction.
// Mapping.  The lanes that serve a context share nothing with any other context.  Where four contexts' slices fit the
// 64 KB of LDS a workgroup may ask for, one wave serves one context and a workgroup is CTXT_WAVES such waves (no
// workgroup barrier); where they do not (large D x N), a workgroup serves one context with all its waves (TEAM).  Either
// way every output element is computed by one lane in full, so the two mappings give the same bits.  A context holds,
// in its slice (the layout of ctxt_slice_floats, flow_ctx_bwd.hip),
//   zs (N, D)          the state: the forward's output z on entry, the draw omega at the end
//   gs (N, D)          the gradient with respect to the state: g_z on entry (0 where it is NULL), g_omega at the end
//   gl (N)             the cotangent of the summed log-det, g_sld (0 where it is NULL)
//   wb                 the block of the context's parameter row the current layer needs (the lower layer with the
//                      stage's Affine block behind it, or the upper layer)
//   act (2, L, N, U)   the tanh outputs of the twin nets; overwritten in place by the deltas on the way back
//   ts (2, N, D - h)   t and s, then their deltas
// and walks the bijectors last to first -- the reverse of the order the sampling pass evaluated them in.  Each stage is
// undone as: the Affine block, BatchNorm c1, the lower coupling layer, BatchNorm c0, the upper coupling layer.  At a
// coupling layer it recomputes the twin nets from the conditioner half (which the layer leaves unchanged), rebuilds the
// layer's input x2 <- (y2 - t) e^-s (the inverse map), sends the deltas back through the transposed weights, contracts
// activations with deltas over the context's samples and writes each weight and bias gradient once, at the slot the
// parameter has in the row.  BatchNorm maps are constants (the shared (2S, D) statistics: no gradient).
//
// Arithmetic.  Plain float32 fused multiply-adds on the layer's real widths (h = D / 2 and D - h, U units): nothing is
// padded.  Every sum over a context's samples is a sequential loop n = 0 .. N-1 in one lane: bit-reproducible, and
// independent of the other contexts of the call.
//
// Writes.  Each of the flow_layout(D, S, L, U).total slots of a gradient row is written exactly once, by one lane of
// those that own the context; no atomics, no workspace; columns beyond the parameter count are not touched.
#include <atomic>

#include "launch.h"
#include "../../include/tnf_ctxsample.h"

namespace tnf {

constexpr int CTXS_WAVES = 4;           // waves per workgroup: one context each, or all on one context (TEAM)
constexpr int CTXS_LDS_BYTES = 65536;   // dynamic LDS of one workgroup

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

// floats of one context's slice: zs, gs, gl, wb, act, ts -- the layout of ctxt_slice_floats (flow_ctx_bwd.hip)
static int64_t ctxs_slice_floats(int N, int D, int S, int L, int U) {
    const FlowLayout fl = flow_layout(D, S, L, U);
    const int64_t wb = fl.p_up > fl.p_low + 2 * D ? fl.p_up : fl.p_low + 2 * D;
    const int64_t n = 2 * (int64_t)N * D + N + wb + 2 * (int64_t)L * N * U + 2 * (int64_t)N * (D - D / 2);
    return (n + 3) & ~(int64_t)3;
}

// The lanes that serve a context exchange values through its LDS slice: everything written before this point is
// visible to every one of them after it.  TEAM: a workgroup barrier.  Otherwise one wave, which runs in lockstep and
// whose LDS operations complete in order: an ordering for the compiler only, and nothing synchronises across waves.
template <bool TEAM>
__device__ __forceinline__ void ctxs_sync() {
    if (TEAM) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// One coupling layer of the walk.  w: the layer's block in LDS, g: its block of the gradient row (global).
// c_off / t_off: where the conditioner half (width din) and the transformed half (width dout) start inside a row.
// t / nt: this lane's index among the nt lanes that serve the context.  Every output element is computed by one lane in
// full, so the results do not depend on nt.  Everything but the step marked "the layer itself" is ctxt_coupling of
// flow_ctx_bwd.hip.
template <bool TEAM>
__device__ __forceinline__ void ctxs_coupling(const float* w, float* __restrict__ g, float* zs, float* gs, const float* gl,
                                              float* act, float* ts, int N, int D, int L, int U, int din, int dout,
                                              int c_off, int t_off, int t, int nt) {
    const int NU = N * U, ND = N * dout;
    const int n_w0 = din * U, n_wh = U * U, n_w2 = U * dout;
    const int sz0 = 2 * n_w0 + 2 * U, szh = 2 * n_wh + 2 * U;
    const float* w2 = w + sz0 + (L - 1) * szh;  // the output layer's [W_t | W_s | b_t | b_s]
    float* g2 = g + sz0 + (L - 1) * szh;

    // ---- forward: first layer, din -> U, tanh.  item (net, n, u); lanes run along u
    for (int i = t; i < 2 * NU; i += nt) {
        const int net = i >= NU, r = i - net * NU, n = r / U, u = r - n * U;
        const float* wn = w + net * n_w0 + u;
        const float* x = zs + n * D + c_off;
        float acc = w[2 * n_w0 + net * U + u];
        for (int f = 0; f < din; ++f) acc = __builtin_fmaf(x[f], wn[f * U], acc);
        act[net * L * NU + r] = tanhf(acc);
    }
    ctxs_sync<TEAM>();
    // ---- hidden layers, U -> U, tanh
    for (int l = 1; l < L; ++l) {
        const float* wl = w + sz0 + (l - 1) * szh;
        for (int i = t; i < 2 * NU; i += nt) {
            const int net = i >= NU, r = i - net * NU, n = r / U, u = r - n * U;
            const float* wn = wl + net * n_wh + u;
            const float* a = act + (net * L + l - 1) * NU + n * U;
            float acc = wl[2 * n_wh + net * U + u];
            for (int k = 0; k < U; ++k) acc = __builtin_fmaf(a[k], wn[k * U], acc);
            act[(net * L + l) * NU + r] = tanhf(acc);
        }
        ctxs_sync<TEAM>();
    }
    // ---- output layer, U -> dout, linear: t and s.  item (net, n, o)
    for (int i = t; i < 2 * ND; i += nt) {
        const int net = i >= ND, r = i - net * ND, n = r / dout, o = r - n * dout;
        const float* wn = w2 + net * n_w2 + o;
        const float* a = act + (net * L + L - 1) * NU + n * U;
        float acc = w2[2 * n_w2 + net * dout + o];
        for (int k = 0; k < U; ++k) acc = __builtin_fmaf(a[k], wn[k * dout], acc);
        ts[i] = acc;
    }
    ctxs_sync<TEAM>();
    // ---- the layer itself.  Sampling ran y2 = t + x2 e^s; with G the gradient at (x1, y2) and gl at sum(s):
    //      rebuild x2 = (y2 - t) e^-s;  G(x2) = G2 e^s;  d t = G2;  d s = G2 x2 e^s + gl
    for (int i = t; i < ND; i += nt) {
        const int n = i / dout, o = i - n * dout;
        const int at = n * D + t_off + o;
        const float tv = ts[i], s = ts[ND + i];
        const float y2 = zs[at], G2 = gs[at];
        const float x2 = (y2 - tv) * expf(-s);
        const float gx = G2 * expf(s);
        zs[at] = x2;
        gs[at] = gx;
        ts[i] = G2;
        ts[ND + i] = __builtin_fmaf(gx, x2, gl[n]);
    }
    ctxs_sync<TEAM>();
    // ---- output layer back: dW2[k][o] = sum_n h[n][k] d[n][o], db2[o] = sum_n d[n][o]
    for (int i = t; i < 2 * n_w2; i += nt) {
        const int net = i >= n_w2, r = i - net * n_w2, k = r / dout, o = r - k * dout;
        const float* a = act + (net * L + L - 1) * NU + k;
        const float* d = ts + net * ND + o;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc = __builtin_fmaf(a[n * U], d[n * dout], acc);
        g2[i] = acc;
    }
    for (int i = t; i < 2 * dout; i += nt) {
        const int net = i >= dout, o = i - net * dout;
        const float* d = ts + net * ND + o;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += d[n * dout];
        g2[2 * n_w2 + i] = acc;
    }
    ctxs_sync<TEAM>();
    // ---- delta of the last hidden activation, in place: d a[n][k] = (sum_o W2[k][o] d[n][o]) (1 - h^2).  Lanes run
    // along k, so the weight reads are dout apart: each lane starts its sum at o = k (rotation) to spread the banks
    for (int i = t; i < 2 * NU; i += nt) {
        const int net = i >= NU, r = i - net * NU, n = r / U, k = r - n * U;
        const float* wn = w2 + net * n_w2 + k * dout;
        const float* d = ts + net * ND + n * dout;
        float acc = 0.f;
        int o = k < dout ? k : 0;
        for (int c = 0; c < dout; ++c) {
            acc = __builtin_fmaf(wn[o], d[o], acc);
            if (++o == dout) o = 0;
        }
        float* hp = act + (net * L + L - 1) * NU + r;
        const float h = *hp;
        *hp = acc * __builtin_fmaf(-h, h, 1.f);
    }
    ctxs_sync<TEAM>();
    // ---- hidden layers back, last to first
    for (int l = L - 1; l >= 1; --l) {
        const float* wl = w + sz0 + (l - 1) * szh;
        float* gw = g + sz0 + (l - 1) * szh;
        for (int i = t; i < 2 * n_wh; i += nt) {  // dWh[k][u] = sum_n h_{l-1}[n][k] d_l[n][u]
            const int net = i >= n_wh, r = i - net * n_wh, k = r / U, u = r - k * U;
            const float* a = act + (net * L + l - 1) * NU + k;
            const float* d = act + (net * L + l) * NU + u;
            float acc = 0.f;
            for (int n = 0; n < N; ++n) acc = __builtin_fmaf(a[n * U], d[n * U], acc);
            gw[i] = acc;
        }
        for (int i = t; i < 2 * U; i += nt) {
            const int net = i >= U, u = i - net * U;
            const float* d = act + (net * L + l) * NU + u;
            float acc = 0.f;
            for (int n = 0; n < N; ++n) acc += d[n * U];
            gw[2 * n_wh + i] = acc;
        }
        ctxs_sync<TEAM>();
        for (int i = t; i < 2 * NU; i += nt) {  // d a_{l-1}[n][k] = (sum_u Wh[k][u] d_l[n][u]) (1 - h^2), in place
            const int net = i >= NU, r = i - net * NU, n = r / U, k = r - n * U;
            const float* wn = wl + net * n_wh + k * U;
            const float* d = act + (net * L + l) * NU + n * U;
            float acc = 0.f;
            int u = k;
            for (int c = 0; c < U; ++c) {
                acc = __builtin_fmaf(wn[u], d[u], acc);
                if (++u == U) u = 0;
            }
            float* hp = act + (net * L + l - 1) * NU + r;
            const float h = *hp;
            *hp = acc * __builtin_fmaf(-h, h, 1.f);
        }
        ctxs_sync<TEAM>();
    }
    // ---- first layer back: dW0[f][u] = sum_n x[n][f] d_0[n][u], db0, and the conditioner half's gradient
    for (int i = t; i < 2 * n_w0; i += nt) {
        const int net = i >= n_w0, r = i - net * n_w0, f = r / U, u = r - f * U;
        const float* x = zs + c_off + f;
        const float* d = act + net * L * NU + u;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc = __builtin_fmaf(x[n * D], d[n * U], acc);
        g[i] = acc;
    }
    for (int i = t; i < 2 * U; i += nt) {
        const int net = i >= U, u = i - net * U;
        const float* d = act + net * L * NU + u;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += d[n * U];
        g[2 * n_w0 + i] = acc;
    }
    for (int i = t; i < N * din; i += nt) {  // G1 += sum_u W0_t[f][u] d_t[n][u] + W0_s[f][u] d_s[n][u]
        const int n = i / din, f = i - n * din;
        const float* wt = w + f * U;
        const float* dt = act + n * U;
        const float* ds = act + L * NU + n * U;
        float acc = gs[n * D + c_off + f];
        int u = f < U ? f : f % U;
        for (int c = 0; c < U; ++c) {
            acc = __builtin_fmaf(wt[u], dt[u], acc);
            acc = __builtin_fmaf(wt[n_w0 + u], ds[u], acc);
            if (++u == U) u = 0;
        }
        gs[n * D + c_off + f] = acc;
    }
    ctxs_sync<TEAM>();
}

// The stage's Affine block, where the walk meets one, and the parameter-free BatchNorm layer in front of it, undone in
// that order:
//   Affine:             sampling ran y = x e^a + shift, so x = (y - shift) e^-a, G(x) = G(y) e^a,
//                       d shift = sum_n G(y), d a = sum_n (G(y) x e^a + gl)
//   BatchNorm (frozen): sampling ran y = (x - mu) / alpha, so x = y alpha + mu and G(x) = G(y) / alpha
// ap / ga: the Affine block [a (D) | shift (D)] in LDS and its gradient slots, or NULL.  One lane per feature: the sums
// over the samples are sequential.
template <bool TEAM>
__device__ __forceinline__ void ctxs_between(const float* __restrict__ mean, const float* __restrict__ alpha, const float* ap,
                                             float* __restrict__ ga, float* zs, float* gs, const float* gl, int N, int D,
                                             int t, int nt) {
    for (int d = t; d < D; d += nt) {
        const float mu = mean[d], al = alpha[d];
        float sh = 0.f, ea = 1.f, ema = 1.f;
        if (ap) {
            const float a = ap[d];
            sh = ap[D + d];
            ea = expf(a);
            ema = expf(-a);
        }
        float da = 0.f, dsh = 0.f;
        for (int n = 0; n < N; ++n) {
            float x = zs[n * D + d], G = gs[n * D + d];
            if (ap) {
                dsh += G;
                x = (x - sh) * ema;
                G *= ea;
                da += __builtin_fmaf(G, x, gl[n]);
            }
            zs[n * D + d] = __builtin_fmaf(x, al, mu);
            gs[n * D + d] = G / al;
        }
        if (ap) {
            ga[d] = da;
            ga[D + d] = dsh;
        }
    }
    ctxs_sync<TEAM>();
}

template <bool TEAM>
__global__ void __launch_bounds__(CTXS_WAVES * 64) ctx_sample_bwd_kernel(CtxSampleArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float ctxs_lds[];
    // TEAM: the workgroup's CTXS_WAVES waves serve one context together; else one wave per context
    const int wave = TEAM ? 0 : __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t = TEAM ? threadIdx.x : threadIdx.x & 63, nt = TEAM ? CTXS_WAVES * 64 : 64;
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
    ctxs_sync<TEAM>();

    for (int st = a.S - 1; st >= 0; --st) {
        const float* ps = p + st * fl.stage;
        float* gst = gp + st * fl.stage;
        const int c0 = 2 * st, c1 = 2 * st + 1;
        // the Affine block and BatchNorm c1, then the lower layer in front of them: conditioner = the last D - h features
        for (int i = t; i < n_low; i += nt) wb[i] = ps[fl.p_up + i];
        ctxs_sync<TEAM>();
        ctxs_between<TEAM>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, wb + fl.p_low, gst + fl.p_up + fl.p_low, zs, gs, gl, N, D,
                           t, nt);
        ctxs_coupling<TEAM>(wb, gst + fl.p_up, zs, gs, gl, act, ts, N, D, L, U, hh, h, h, 0, t, nt);
        // BatchNorm c0, then the upper layer: conditioner = the first h features, transformed = the other D - h
        for (int i = t; i < n_up; i += nt) wb[i] = ps[i];
        ctxs_between<TEAM>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, nullptr, nullptr, zs, gs, gl, N, D, t, nt);
        ctxs_coupling<TEAM>(wb, gst, zs, gs, gl, act, ts, N, D, L, U, h, hh, 0, h, t, nt);
    }

    if (a.g_omega) {
        float* go = a.g_omega + m * (int64_t)N * D;
        for (int i = t; i < N * D; i += nt) go[i] = gs[i];
    }
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_sample_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return D >= 2 && D <= 64 && S >= 1 && L >= 1 && L <= 3 && U >= 1 && U <= 16 && N >= 1 && N <= 31 ? 1 : 0;
}

int64_t tnf_ctx_sample_launch_count(void) { return g_ctxsample_launches.load(std::memory_order_relaxed); }

int tnf_ctx_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha, const float* g_z,
                           const float* g_sld, float* g_params, float* g_omega, int64_t M, int64_t N, int32_t D, int32_t S,
                           int32_t L, int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_ctx_sample_bwd_f32";
    if (!z || !params || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: no upstream gradient (g_z and g_sld both NULL)", fn);
    if (M < 1 || N < 0) return fail(TNF_EINVAL, "%s: M=%lld N=%lld", fn, (long long)M, (long long)N);
    if (M > (int64_t)0x7fffffff) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!tnf_ctx_sample_supported(D, S, L, U, N == 0 ? 1 : N))
        return fail(TNF_EUNSUPPORTED, "%s: no per-context kernel for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L, U, (long long)N);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    if (gpstride < need)
        return fail(TNF_EINVAL, "%s: gradient row has %lld elements, flow needs %lld", fn, (long long)gpstride, (long long)need);
    if (g_omega && (g_omega == z || g_omega == g_z)) return fail(TNF_EINVAL, "%s: g_omega must not alias z or g_z", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (N == 0) return TNF_OK;
    // CTXS_WAVES contexts per workgroup, one wave each, where four slices fit the workgroup's LDS; else one context per
    // workgroup, served by all its waves (large D x N: few contexts fit a CU, each with enough elements for 256 lanes)
    const int64_t slice = ctxs_slice_floats((int)N, D, S, L, U);
    if (slice * 4 > CTXS_LDS_BYTES)
        return fail(TNF_EUNSUPPORTED, "%s: a context's slice (%lld bytes) exceeds the workgroup's LDS", fn, (long long)(slice * 4));
    const bool team = CTXS_WAVES * slice * 4 > CTXS_LDS_BYTES;
    const CtxSampleArgs a{z, params, bn_mean, bn_alpha, g_z, g_sld, g_params, g_omega, M, pstride, gpstride, (int)N, D, S, L, U,
                          (int)slice, g_launch_gate};
    g_ctxsample_launches.fetch_add(1, std::memory_order_relaxed);
    if (team)
        hipLaunchKernelGGL(ctx_sample_bwd_kernel<true>, dim3((unsigned)M), dim3(CTXS_WAVES * 64), (size_t)(slice * 4),
                           as_stream(stream), a);
    else
        hipLaunchKernelGGL(ctx_sample_bwd_kernel<false>, dim3((unsigned)((M + CTXS_WAVES - 1) / CTXS_WAVES)),
                           dim3(CTXS_WAVES * 64), (size_t)(CTXS_WAVES * slice * 4), as_stream(stream), a);
    return check_launch("ctx_sample_bwd");
}

}  // extern "C"
