// What the two per-context backward kernels share: ctx_train_bwd_kernel (flow_ctx_bwd.hip, the backward of log_prob) and
// ctx_sample_bwd_kernel (flow_ctx_sample_bwd.hip, the backward of frozen-statistics sampling) walk the same flow in
// opposite directions, over the same slice, with the same mapping.  A file keeps what has a direction; the rest is here.
//
// Mapping.  The lanes that serve a context share nothing with any other context.  Where four contexts' slices fit the
// 64 KB of LDS a workgroup may ask for, one wave serves one context and a workgroup is CTX_BWD_WAVES such waves (no
// workgroup barrier).  Where they do not (large D x N), a workgroup serves one context with all its waves (TEAM): few
// contexts fit a CU then, and each has enough elements per step for 256 lanes (one wave per context there
// left a CU with three waves and lost to the composition at N = 31).  Either way every output element is computed by one
// lane in full, so the two mappings give the same bits.
//
// Slice.  A context holds, in LDS,
//   zs (N, D)          the state
//   gs (N, D)          the gradient with respect to the state
//   gl (N)             the cotangent of the summed log-det
//   wb                 the block of the context's parameter row the current layer needs (the upper layer, or the lower
//                      layer with the stage's Affine block behind it)
//   act (2, L, N, U)   the tanh outputs of the twin nets; overwritten in place by the deltas on the way back
//   ts (2, N, D - h)   t and s, then their deltas
// in this order; what zs, gs and gl hold on entry and at the end is the direction's (see each file).
//
// Arithmetic.  Plain float32 fused multiply-adds on the layer's real widths (h = D / 2 and D - h, U units): there is no
// tile to pad, so no padded sample, feature or unit exists anywhere -- rows beyond N, the odd half and a 16th unit at
// U = 15 have nothing to contribute because they are never formed.  Every sum over a context's samples is a sequential
// loop n = 0 .. N-1 in one lane: bit-reproducible, and independent of the other contexts of the call.  Why not the MFMA
// tile of the forward: with the sample index as the K index of the weight-gradient contraction, N <= 31 samples fill a
// 16-wide tile to 1/16 .. 1/2, and the launch is bound by the rows it moves -- a row and its gradient row are 2 x 82 KB
// per context at D = 64, S = 4 against ~0.5 M multiply-adds at N = 8.
//
// Writes.  Each of the flow_layout(D, S, L, U).total slots of a gradient row is written exactly once, by one lane of
// those that own the context; no atomics, no workspace; columns beyond the parameter count are not touched.
#pragma once
#include <atomic>

#include "launch.h"

namespace tnf {

constexpr int CTX_BWD_WAVES = 4;           // waves per workgroup: one context each, or all on one context (TEAM)
constexpr int CTX_BWD_LDS_BYTES = 65536;   // dynamic LDS of one workgroup

// floats of one context's slice (host and device agree through the kernel argument `slice`)
static int64_t ctx_bwd_slice_floats(int N, int D, int S, int L, int U) {
    const FlowLayout fl = flow_layout(D, S, L, U);
    const int64_t wb = fl.p_up > fl.p_low + 2 * D ? fl.p_up : fl.p_low + 2 * D;
    const int64_t n = 2 * (int64_t)N * D + N + wb + 2 * (int64_t)L * N * U + 2 * (int64_t)N * (D - D / 2);
    return (n + 3) & ~(int64_t)3;
}

// The lanes that serve a context exchange values through its LDS slice: everything written before this point is
// visible to every one of them after it.  TEAM: the context has the whole workgroup (one context per workgroup), a
// workgroup barrier.  Otherwise one wave, which runs in lockstep and whose LDS operations complete in order: an ordering
// for the compiler only (no instruction beyond the wait the reads need anyway), and nothing synchronises across waves.
template <bool TEAM>
__device__ __forceinline__ void ctx_bwd_sync() {
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
// full, so the results do not depend on nt.  STEP::apply is the layer itself, for one element of the transformed half:
// from t = ts[i], s = ts[ND + i], the state zs[at], its gradient gs[at] and the log-det cotangent gl[n] it rebuilds the
// layer's input in zs[at], that input's gradient in gs[at], and leaves the deltas of t and s in ts[i] and ts[ND + i].
template <bool TEAM, class STEP>
__device__ __forceinline__ void ctx_bwd_coupling(const float* w, float* __restrict__ g, float* zs, float* gs,
                                                 const float* gl, float* act, float* ts, int N, int D, int L, int U,
                                                 int din, int dout, int c_off, int t_off, int t, int nt) {
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
    ctx_bwd_sync<TEAM>();
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
        ctx_bwd_sync<TEAM>();
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
    ctx_bwd_sync<TEAM>();
    // ---- the layer itself
    for (int i = t; i < ND; i += nt) {
        const int n = i / dout, o = i - n * dout;
        const int at = n * D + t_off + o;
        STEP::apply(zs, gs, gl, ts, ND, i, at, n);
    }
    ctx_bwd_sync<TEAM>();
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
    ctx_bwd_sync<TEAM>();
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
    ctx_bwd_sync<TEAM>();
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
        ctx_bwd_sync<TEAM>();
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
        ctx_bwd_sync<TEAM>();
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
    ctx_bwd_sync<TEAM>();
}

// Host side.  The domain of both kernels: every supported shape's slice fits one workgroup, so no resource fall-back.
inline int ctx_bwd_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return D >= 2 && D <= 64 && S >= 1 && L >= 1 && L <= 3 && U >= 1 && U <= 16 && N >= 1 && N <= 31 ? 1 : 0;
}

// The checks of the shape and the two row strides that both entries make, in their order; N = 0 is a shape like any
// other here (the entry returns TNF_OK for it only after every check).
inline int ctx_bwd_check(const char* fn, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U,
                         int64_t pstride, int64_t gpstride) {
    if (M < 1 || N < 0) return fail(TNF_EINVAL, "%s: M=%lld N=%lld", fn, (long long)M, (long long)N);
    if (M > (int64_t)0x7fffffff) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!ctx_bwd_supported(D, S, L, U, N == 0 ? 1 : N))
        return fail(TNF_EUNSUPPORTED, "%s: no per-context kernel for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L, U, (long long)N);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    if (gpstride < need)
        return fail(TNF_EINVAL, "%s: gradient row has %lld elements, flow needs %lld", fn, (long long)gpstride, (long long)need);
    return TNF_OK;
}

// Launch `a` (its shape filled in, its slice not yet) under the mapping its slice allows: one wave per context where
// CTX_BWD_WAVES slices fit the workgroup's LDS, else TEAM.  `launches` is the entry's counter.
template <class ARGS>
int ctx_bwd_launch(const char* fn, const char* name, void (*per_wave)(ARGS), void (*team)(ARGS), ARGS a,
                   std::atomic<long long>& launches, void* stream) {
    const int64_t slice = ctx_bwd_slice_floats(a.N, a.D, a.S, a.L, a.U);
    if (slice * 4 > CTX_BWD_LDS_BYTES)
        return fail(TNF_EUNSUPPORTED, "%s: a context's slice (%lld bytes) exceeds the workgroup's LDS", fn, (long long)(slice * 4));
    a.slice = (int)slice;
    launches.fetch_add(1, std::memory_order_relaxed);
    if (CTX_BWD_WAVES * slice * 4 > CTX_BWD_LDS_BYTES)
        hipLaunchKernelGGL(team, dim3((unsigned)a.M), dim3(CTX_BWD_WAVES * 64), (size_t)(slice * 4), as_stream(stream), a);
    else
        hipLaunchKernelGGL(per_wave, dim3((unsigned)((a.M + CTX_BWD_WAVES - 1) / CTX_BWD_WAVES)), dim3(CTX_BWD_WAVES * 64),
                           (size_t)(CTX_BWD_WAVES * slice * 4), as_stream(stream), a);
    return check_launch(name);
}

}  // namespace tnf
