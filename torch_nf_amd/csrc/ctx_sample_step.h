// The sampling direction of the per-context walk (ctx_bwd_walk.h), shared by the two backward kernels of frozen-statistics
// sampling: ctx_sample_bwd_kernel (flow_ctx_sample_bwd.hip, up to 16 units) and ctx_wide_sample_bwd_kernel
// (flow_ctx_wide_sample_bwd.hip, 17 .. 64 units).  Both undo a stage as: the Affine block, BatchNorm c1, the lower
// coupling layer, BatchNorm c0, the upper coupling layer.
#pragma once
#include "ctx_bwd_walk.h"

namespace tnf {

// The coupling layer itself (ctx_bwd_coupling's STEP).  Sampling ran y2 = t + x2 e^s; with G the gradient at (x1, y2)
// and gl at sum(s):  rebuild x2 = (y2 - t) e^-s;  G(x2) = G2 e^s;  d t = G2;  d s = G2 x2 e^s + gl
struct CtxSampleStep {
    static __device__ __forceinline__ void apply(float* zs, float* gs, const float* gl, float* ts, int ND, int i, int at,
                                                 int n) {
        const float tv = ts[i], s = ts[ND + i];
        const float y2 = zs[at], G2 = gs[at];
        const float x2 = (y2 - tv) * expf(-s);
        const float gx = G2 * expf(s);
        zs[at] = x2;
        gs[at] = gx;
        ts[i] = G2;
        ts[ND + i] = __builtin_fmaf(gx, x2, gl[n]);
    }
};

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
    ctx_bwd_sync<TEAM>();
}

}  // namespace tnf
