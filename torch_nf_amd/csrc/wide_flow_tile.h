// The whole-flow form of the "wide" fp32-MFMA coupling tile (flow_wide.hip): the LDS budget and support predicate, the
// operand image of wide_tile.h generalised to a layer whose input and output widths differ, and one coupling layer on a
// 16-sample tile held in registers.
//
// LDS of one workgroup, in floats (restated by tests/wideflow_restatement.py):
//     per coupling layer   WideLayout{UT, HT, L}.floats()        the folded operand image, HT = ceil(ceil(D / 2) / 16)
//                        + 64 * HT                               the fold constants [A_lo | A_hi | B_lo | B_hi], 16 HT each
//     wide_flow_lds_bytes(D, S, L, U) = 4 * 2 S * (floats() + 64 HT)
// wide_flow_supported(D, S, L, U): 2 <= D <= 64, S >= 1, 1 <= L <= 5, 17 <= U <= 64 and
//     wide_flow_lds_bytes(D, S, L, U) <= 150 KB (153,600 B, the budget of wide_supported).
#pragma once
#include "wide_tile.h"

namespace tnf {

constexpr int64_t kWideFlowLdsBudget = 150 * 1024;

inline WideLayout wide_flow_layout(int D, int L, int U) {
    WideLayout wl;
    wl.UT = (U + 15) / 16;
    wl.HT = ((D + 1) / 2 + 15) / 16;
    wl.L = L;
    return wl;
}
// floats per coupling layer: image + fold constants
inline int64_t wide_flow_layer_floats(int D, int L, int U) {
    const WideLayout wl = wide_flow_layout(D, L, U);
    return (int64_t)wl.floats() + 64 * wl.HT;
}
inline int64_t wide_flow_lds_bytes(int D, int S, int L, int U) { return 4 * 2 * (int64_t)S * wide_flow_layer_floats(D, L, U); }
inline bool wide_flow_supported(int D, int S, int L, int U) {
    if (D < 2 || D > 64 || S < 1 || L < 1 || L > 5 || U < 17 || U > 64) return false;
    if (S > 64) return false;  // (no image of any shape fits 128 times; keeps the product below in range)
    return wide_flow_lds_bytes(D, S, L, U) <= kWideFlowLdsBudget;
}

#if defined(__HIPCC__)
// build_wide_image of wide_tile.h for a layer d_in -> U -> ... -> U -> d_out (bijectors.py:222-235), both widths zero-
// padded to 16 HT: the first layer's weight rows f >= d_in and the output layer's weight columns and biases o >= d_out
// are zero in the image.  The work is cut into units that share nothing -- one (net, 16 output units) block of one MLP
// layer each, its column sums included -- and `unit` counts them across calls: wave `wave` of `nwaves` builds the units
// with unit % nwaves == wave, so a workgroup builds the images of all its layers in one balanced pass.  Full waves only
// (the column sums use cross-lane shuffles); `wave` is wave-uniform.
__device__ inline void build_wide_image_io(float* img, const float* __restrict__ p, WideLayout wl, int d_in, int d_out,
                                           int U, int lane, int wave, int nwaves, int& unit) {
    const int r = lane & 15, q = lane >> 4;
    float* wdst = img + lane * 4;
    float* bdst = img + wl.NWG() * 256 + q * 4;
    const bool bias_lane = r == 0;
    // layer 0: d_in -> U, feeds a tanh: weights and biases scaled by c = 2 log2(e)
    {
        const float* w[2] = {p, p + d_in * U};
        const float* b[2] = {p + 2 * d_in * U, p + 2 * d_in * U + U};
        for (int net = 0; net < 2; ++net)
            for (int ut = 0; ut < wl.UT; ++ut) {
                if (unit++ % nwaves != wave) continue;
                const int u = 16 * ut + r;
                for (int m = 0; m < wl.HT; ++m) {
                    f4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int f = 16 * m + 4 * q + j;
                        v[j] = kTwoLog2e * ld_sel(w[net], f * U + u, f < d_in && u < U);
                    }
                    *reinterpret_cast<f4*>(wdst + wl.g_w0(net, ut, m) * 256) = v;
                }
                f4 bv;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ub = 16 * ut + 4 * q + j;
                    bv[j] = kTwoLog2e * ld_sel(b[net], ub, ub < U);
                }
                if (bias_lane) *reinterpret_cast<f4*>(bdst + wl.b_b0(net, ut) * 16) = bv;
            }
        p += 2 * d_in * U + 2 * U;
    }
    // hidden layers: U -> U, consume r = (1 - tanh)/2, feed a tanh
    for (int l = 0; l < wl.L - 1; ++l) {
        const float* w[2] = {p, p + U * U};
        const float* b[2] = {p + 2 * U * U, p + 2 * U * U + U};
        for (int net = 0; net < 2; ++net)
            for (int uo = 0; uo < wl.UT; ++uo) {
                if (unit++ % nwaves != wave) continue;
                const int o = 16 * uo + r;
                float csum = 0.f;
                for (int ui = 0; ui < wl.UT; ++ui) {
                    f4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 16 * ui + 4 * q + j;
                        const float raw = ld_sel(w[net], k * U + o, k < U && o < U);
                        csum += raw;
                        v[j] = -2.f * kTwoLog2e * raw;
                    }
                    *reinterpret_cast<f4*>(wdst + wl.g_wh(l, net, uo, ui) * 256) = v;
                }
                csum = reduce_q(csum);  // column sum of W for output unit 16uo + r
                f4 bv;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ob = 16 * uo + 4 * q + j;
                    const float cs = __shfl(csum, 4 * q + j);
                    bv[j] = ob < U ? kTwoLog2e * (ld_sel(b[net], ob, ob < U) + cs) : 0.f;
                }
                if (bias_lane) *reinterpret_cast<f4*>(bdst + wl.b_bh(l, net, uo) * 16) = bv;
            }
        p += 2 * U * U + 2 * U;
    }
    // output layer: U -> d_out, consumes r; t plain, s scaled by log2(e)
    {
        const float* w[2] = {p, p + U * d_out};
        const float* b[2] = {p + 2 * U * d_out, p + 2 * U * d_out + d_out};
        for (int net = 0; net < 2; ++net) {
            const float sc = net == 0 ? 1.f : kLog2e;
            for (int mo = 0; mo < wl.HT; ++mo) {
                if (unit++ % nwaves != wave) continue;
                const int o = 16 * mo + r;
                float csum = 0.f;
                for (int ui = 0; ui < wl.UT; ++ui) {
                    f4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 16 * ui + 4 * q + j;
                        const float raw = ld_sel(w[net], k * d_out + o, k < U && o < d_out);
                        csum += raw;
                        v[j] = -2.f * sc * raw;
                    }
                    *reinterpret_cast<f4*>(wdst + wl.g_w2(net, mo, ui) * 256) = v;
                }
                csum = reduce_q(csum);
                f4 bv;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ob = 16 * mo + 4 * q + j;
                    const float cs = __shfl(csum, 4 * q + j);
                    bv[j] = ob < d_out ? sc * (ld_sel(b[net], ob, ob < d_out) + cs) : 0.f;
                }
                if (bias_lane) *reinterpret_cast<f4*>(bdst + wl.b_b2(net, mo) * 16) = bv;
            }
        }
    }
}

// r = 1 / (2^a + 1) as sig2 of wave_prims.h, with one Newton step on v_rcp_f32's result: r' = r + r (1 - d r).  The
// activation's error is what a deep net amplifies: every tanh layer feeds the next, and the last one feeds e^(+-s).  The
// step halves the reciprocal's share of that error for three vector instructions per activation, which cost 6-13 % of the
// kernel's time at L = 2 (the exp2 / rcp sections bind it beside the MFMAs), so it is taken for deep nets only: L >= 4
// (DEEP), where the error has four or five dependent activation stages per coupling layer to grow through; up to L = 3
// the plain form has 1.7 x of room under the float64 bars.  The clamp keeps d finite, so that 1 - d r is
// never inf * 0 (r is then 2^-126 or flushed to 0: the value sig2 gives).
__device__ __forceinline__ float sig2_nr(float a) {
    const float d = __builtin_amdgcn_exp2f(fminf(a, 126.f)) + 1.0f;
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ f4 sig2_nr4(f4 v) { return f4{sig2_nr(v[0]), sig2_nr(v[1]), sig2_nr(v[2]), sig2_nr(v[3])}; }

// One coupling layer on one 16-sample tile, operands from the layer's LDS image: the body of coupling_wide_kernel.
// x = conditioner half (unchanged), y = transformed half (updated in place), ssum += this lane's share of
// sum(s) log2(e).  Padded slots of y get t = 0, s' = 0: (0 - 0) 2^-0 = 0 inverse, 0 2^0 + 0 = 0 forward.
template <int HT, int UT, bool INV, bool DEEP>
__device__ __forceinline__ void wide_flow_layer(const float* img, const WideLayout& wl, int lane, const f4 (&x)[HT],
                                                f4 (&y)[HT], float& ssum) {
    const float* wsrc = img + lane * 4;
    const float* bsrc = img + wl.NWG() * 256 + (lane >> 4) * 4;
    auto wgrp = [&](int g) -> f4 { return *reinterpret_cast<const f4*>(wsrc + g * 256); };
    auto bgrp = [&](int g) -> f4 { return *reinterpret_cast<const f4*>(bsrc + g * 16); };
    auto act = [](f4 v) -> f4 {
        if constexpr (DEEP) return sig2_nr4(v);
        else return sig2_4(v);
    };
    f4 rt[UT], rs[UT];
#pragma unroll
    for (int ut = 0; ut < UT; ++ut) {
        f4 at = bgrp(wl.b_b0(0, ut)), as = bgrp(wl.b_b0(1, ut));
#pragma unroll
        for (int mm = 0; mm < HT; ++mm) {
            const f4 wt = wgrp(wl.g_w0(0, ut, mm)), ws = wgrp(wl.g_w0(1, ut, mm));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                at = mfma4(wt[j], x[mm][j], at);
                as = mfma4(ws[j], x[mm][j], as);
            }
        }
        rt[ut] = act(at);
        rs[ut] = act(as);
    }
    for (int l = 0; l < wl.L - 1; ++l) {
        f4 nt[UT], ns[UT];
#pragma unroll
        for (int uo = 0; uo < UT; ++uo) {
            f4 at = bgrp(wl.b_bh(l, 0, uo)), as = bgrp(wl.b_bh(l, 1, uo));
#pragma unroll
            for (int ui = 0; ui < UT; ++ui) {
                const f4 wt = wgrp(wl.g_wh(l, 0, uo, ui)), ws = wgrp(wl.g_wh(l, 1, uo, ui));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    at = mfma4(wt[j], rt[ui][j], at);
                    as = mfma4(ws[j], rs[ui][j], as);
                }
            }
            nt[uo] = act(at);
            ns[uo] = act(as);
        }
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            rt[u] = nt[u];
            rs[u] = ns[u];
        }
    }
#pragma unroll
    for (int mo = 0; mo < HT; ++mo) {
        f4 tt = bgrp(wl.b_b2(0, mo)), sv = bgrp(wl.b_b2(1, mo));
#pragma unroll
        for (int ui = 0; ui < UT; ++ui) {
            const f4 wt = wgrp(wl.g_w2(0, mo, ui)), ws = wgrp(wl.g_w2(1, mo, ui));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                tt = mfma4(wt[j], rt[ui][j], tt);
                sv = mfma4(ws[j], rs[ui][j], sv);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s2 = sv[j];  // 0 for padded features (zero weights and bias)
            ssum += s2;
            if (INV) y[mo][j] = (y[mo][j] - tt[j]) * __builtin_amdgcn_exp2f(-s2);
            else y[mo][j] = __builtin_fmaf(y[mo][j], __builtin_amdgcn_exp2f(s2), tt[j]);
        }
    }
}

// The map between coupling layers on both register halves: v -> v A + B from the layer's fold block
// [A_lo | A_hi | B_lo | B_hi]; a padded slot holds (1, 0) and stays exactly 0.
template <int HT>
__device__ __forceinline__ void wide_flow_fold(const float* fold, int q, f4 (&lo)[HT], f4 (&hi)[HT]) {
#pragma unroll
    for (int mm = 0; mm < HT; ++mm) {
        const int o = 16 * mm + 4 * q;
        const f4 al = *reinterpret_cast<const f4*>(fold + o), ah = *reinterpret_cast<const f4*>(fold + 16 * HT + o);
        const f4 bl = *reinterpret_cast<const f4*>(fold + 32 * HT + o), bh = *reinterpret_cast<const f4*>(fold + 48 * HT + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo[mm][j] = __builtin_fmaf(lo[mm][j], al[j], bl[j]);
            hi[mm][j] = __builtin_fmaf(hi[mm][j], ah[j], bh[j]);
        }
    }
}
#endif  // __HIPCC__

}  // namespace tnf
