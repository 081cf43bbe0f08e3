// Backward of MAF.forward_and_log_det -- the SAMPLING direction (D - 1 sequential passes in the reference) -- in one
// kernel on the matrix pipe (float32, exact-f32 MFMA operands), and the C entries of include/tnf_arsample.h.
//   x solves G(x, theta) = omega,  G(x)_d = (x_d - mu_d(x)) e^-alpha_d(x),  ld = A(x) = sum alpha
//   given g_x (M,N,D), g_ld (M,N):  g_omega (M,N,D),  g_params (M_p, P)
// Implicit differentiation through the inverse-direction backward K (maf_bwd_mfma.hip), rearranged so that everything
// that does not depend on the iterate is done once.  Per 16-sample tile and wave:
//   1. the twin masked MLPs at x, once: mu, e^alpha, e^-alpha and every hidden level's r (tanh' = 4 r (1 - r));
//   2. v <- e^alpha g_x, then D - 1 sweeps  v <- e^alpha (g_x - N(v)),  N(v) the nets' share of K_z(v, -g_ld):
//      deltas d_mu = -v e^-alpha, d_alpha = -v e^-alpha (x - mu) - g_ld (zero on padded features) back through layers
//      L .. 0 with the transposed weight image -- registers and LDS reads only, no weight gradients, no transposes;
//      N is strictly triangular in the autoregressive order and its last column is zero, so D - 1 sweeps are exact;
//   3. one full backward at (x; g_out = v, g_ld' = -g_ld) with the weight-gradient outer products; g_omega = v and
//      g_theta = -K_theta, negated at the flush.
// Layout, image build, LDS sizing, tile walk and flush are those of maf_bwd_mfma_kernel (maf_bwd_tile.h).  The
// accumulators are plain float: v is not bounded by max |g|, so the fixed-point mode has nothing to scale by.
// Fused AR-stack mode (fold != NULL): the rows are z of [MAF, BatchNorm, Affine] with frozen statistics; the load stage
// rebuilds x = z A + B, forms g_x = g_z / A and reduces GZ = sum g_z z, GB = sum g_z, GS = sum g_sld per parameter row.
#include <atomic>

#include "maf_bwd_tile.h"
#include "../../include/tnf_arsample.h"

namespace tnf {

struct MafSampleBwdArgs {
    const float* x;      // the sample (M,N,D); fused mode: the stack's output z
    const float* params;
    const float* masks;
    const float* g_x;    // (M,N,D) or NULL (= zero); fused mode: g_z
    const float* g_ld;   // (M,N) or NULL (= zero); fused mode: g_sld
    float* g_omega;      // (M,N,D) or NULL: not wanted
    float* g_params;
    int64_t M, Mp, N, pstride, gpstride;
    int D, L, U, nacc;
    const float* fold;   // fused mode: A | B per parameter row (launch_ar_fold, inverse), else NULL
    float* g_sums;       // fused mode: (Mp, 2 D + 1) GZ | GB | GS, zeroed by the launcher
};

template <int DT, int UT, bool VEC>
__global__ void __launch_bounds__(256)
maf_sample_bwd_kernel(MafSampleBwdArgs a, MafBLayout wl) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = a.D, U = a.U, L = wl.L;
    const int NWG = wl.NWG();
    float* fimg = lds;
    float* timg = fimg + wl.fwd_floats();
    const int nacc = a.nacc;  // 4: one private copy per wave, plain read-add-write; 1: one shared copy, ds_add_f32
    float* gacc = timg + NWG * 256;
    float* scr_all = gacc + nacc * NWG * 256;
    float* cst = scr_all + 4 * 2 * 272;  // fused mode: fold A | B (2 D), one row of fold sums (2 D + 1) per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, q = lane >> 4;
    float* scrA = scr_all + wave * 2 * 272;
    float* scrB = scrA + 272;
    const int64_t m = grid_m();
    if (m >= a.M) return;
    const int64_t mp = a.Mp == 1 ? 0 : m;
    for (int i = threadIdx.x; i < nacc * NWG * 256; i += 256) gacc[i] = 0.f;
    const bool fusedm = a.fold != nullptr;
    float* red = cst + 2 * D;
    if (fusedm)
        for (int i = threadIdx.x; i < 2 * D; i += 256) cst[i] = a.fold[mp * 2 * D + i];
    build_maf_bwd_images(fimg, timg, a.params + mp * a.pstride, a.masks, wl, D, U, lane, wave, 4, 0);
    __syncthreads();

    const float* fsrc = fimg + lane * 4;
    const float* bsrc = fimg + NWG * 256 + q * 4;
    const float* tsrc = timg + lane * 4;
    float* gdst = gacc + (nacc > 1 ? wave * NWG * 256 : 0) + lane * 4;
    auto wgrp = [&](int g) -> f4 { return *reinterpret_cast<const f4*>(fsrc + g * 256); };
    auto bgrp = [&](int g) -> f4 { return *reinterpret_cast<const f4*>(bsrc + g * 16); };
    auto tgrp = [&](int g) -> f4 { return *reinterpret_cast<const f4*>(tsrc + g * 256); };
    const f4 zero = {0.f, 0.f, 0.f, 0.f};
    auto gadd = [&](int g, f4 v) {
        if (nacc > 1) {
            f4* p = reinterpret_cast<f4*>(gdst + g * 256);
            *p = *p + v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(gdst + g * 256 + j, v[j]);  // ds_add_f32
        }
    };

    const float* xb = a.x + m * a.N * D;
    const float* gxb = a.g_x ? a.g_x + m * a.N * D : nullptr;
    const float* glb = a.g_ld ? a.g_ld + m * a.N : nullptr;
    float* gob = a.g_omega ? a.g_omega + m * a.N * D : nullptr;
    f4 fGZ[DT], fGB[DT];  // fused mode: this lane's share of GZ, GB
    float gs_acc = 0.f;
#pragma unroll
    for (int mm = 0; mm < DT; ++mm) fGZ[mm] = fGB[mm] = zero;

    const int64_t ntiles = (a.N + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t row = tile * 16 + s;
        const bool row_ok = row < a.N;
        const int64_t rr = row_ok ? row : a.N - 1;
        f4 x[DT], g[DT];
#pragma unroll
        for (int mm = 0; mm < DT; ++mm) {
            const int f0 = 16 * mm + 4 * q;
            if (VEC) {
                x[mm] = f0 < D ? *reinterpret_cast<const f4*>(xb + rr * D + f0) : zero;
                g[mm] = (gxb && f0 < D && row_ok) ? *reinterpret_cast<const f4*>(gxb + rr * D + f0) : zero;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[mm][j] = ld_sel(xb + rr * D, f0 + j, f0 + j < D);
                    g[mm][j] = (gxb && row_ok) ? ld_sel(gxb + rr * D, f0 + j, f0 + j < D) : 0.f;
                }
            }
        }
        const float gl = (glb && row_ok) ? glb[rr] : 0.f;
        if (fusedm) {  // the bijectors behind the MAF: z = (x - B) / A
            if (q == 0) gs_acc += gl;
#pragma unroll
            for (int mm = 0; mm < DT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mm + 4 * q + j;
                    fGZ[mm][j] = __builtin_fmaf(g[mm][j], x[mm][j], fGZ[mm][j]);
                    fGB[mm][j] += g[mm][j];
                    if (f < D) {  // (padded features: x = g = 0 already)
                        x[mm][j] = __builtin_fmaf(x[mm][j], cst[f], cst[D + f]);
                        g[mm][j] = g[mm][j] / cst[f];
                    }
                }
        }
        asm volatile("" ::: "memory");

        // ---- 1. the nets at x, once: r of every hidden level, mu, e^-alpha, e^alpha ----
        f4 r[kMafLMax][2][UT];
#pragma unroll
        for (int ut = 0; ut < UT; ++ut) {
            f4 at = zero, as = zero;
#pragma unroll
            for (int mm = 0; mm < DT; ++mm) {
                const f4 wt = wgrp(wl.g0(0, ut, mm)), ws = wgrp(wl.g0(1, ut, mm));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    at = mfma4(wt[j], x[mm][j], at);
                    as = mfma4(ws[j], x[mm][j], as);
                }
            }
            r[0][0][ut] = sig2_4(at);
            r[0][1][ut] = sig2_4(as);
        }
#pragma unroll
        for (int l = 1; l < kMafLMax; ++l) {
            if (l < L) {
#pragma unroll
                for (int uo = 0; uo < UT; ++uo) {
                    f4 at = bgrp(wl.bh(l - 1, 0, uo)), as = bgrp(wl.bh(l - 1, 1, uo));
#pragma unroll
                    for (int ui = 0; ui < UT; ++ui) {
                        const f4 wt = wgrp(wl.gh(l - 1, 0, uo, ui)), ws = wgrp(wl.gh(l - 1, 1, uo, ui));
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            at = mfma4(wt[j], r[l - 1][0][ui][j], at);
                            as = mfma4(ws[j], r[l - 1][1][ui][j], as);
                        }
                    }
                    r[l][0][uo] = sig2_4(at);
                    r[l][1][uo] = sig2_4(as);
                }
            }
        }
        f4 e[DT], ea[DT], xm[DT], v[DT];  // e^-alpha, e^alpha, x - mu, the iterate
#pragma unroll
        for (int mo = 0; mo < DT; ++mo) {
            f4 mu = bgrp(wl.b2(0, mo)), al2 = bgrp(wl.b2(1, mo));
#pragma unroll
            for (int l = 0; l < kMafLMax; ++l) {
                if (l == L - 1) {
#pragma unroll
                    for (int ui = 0; ui < UT; ++ui) {
                        const f4 wt = wgrp(wl.g2(0, mo, ui)), ws = wgrp(wl.g2(1, mo, ui));
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            mu = mfma4(wt[j], r[l][0][ui][j], mu);
                            al2 = mfma4(ws[j], r[l][1][ui][j], al2);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[mo][j] = __builtin_amdgcn_exp2f(-al2[j]);
                ea[mo][j] = __builtin_amdgcn_exp2f(al2[j]);
                xm[mo][j] = x[mo][j] - mu[j];
                v[mo][j] = ea[mo][j] * g[mo][j];
            }
        }
        auto level_r = [&](int lev, int net, int t) -> f4 {  // r of hidden level lev
            f4 o = zero;
#pragma unroll
            for (int l = 0; l < kMafLMax; ++l)
                if (l == lev) o = r[l][net][t];
            return o;
        };

        // One backward pass of the nets at the iterate v.  WG false: a sweep, deltas only, N(v) -> nv.
        // WG true: the last pass, with the weight-gradient outer products of maf_bwd_mfma_kernel section 3
        // (dW[o][k] = sum_s delta[o][s] in[k][s], both operands transposed through the per-wave LDS scratch).
        f4 nv[DT];
        auto back = [&](auto wgc) {
            constexpr bool WG = decltype(wgc)::value;
            f4 dlt[2][DT];
#pragma unroll
            for (int mo = 0; mo < DT; ++mo)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ve = v[mo][j] * e[mo][j];
                    dlt[0][mo][j] = -ve;
                    // padded features (f >= D): v = 0, but g_ld must not leak into them
                    dlt[1][mo][j] = (16 * mo + 4 * q + j < D) ? (-ve * xm[mo][j] - gl) : 0.f;
                }
            f4 dprev[2][UT];
#pragma unroll
            for (int net = 0; net < 2; ++net) {  // output layer: inputs = hidden level L-1, outputs = DT tiles
#pragma unroll
                for (int ui = 0; ui < UT; ++ui) {
                    const f4 rv = level_r(L - 1, net, ui);
                    f4 h_t = zero;
                    if (WG) h_t = transpose_tile(1.f - 2.f * rv, scrB, lane);
                    f4 acc = zero;
#pragma unroll
                    for (int mo = 0; mo < DT; ++mo) {
                        if (WG) {
                            const f4 dt_ = transpose_tile(dlt[net][mo], scrA, lane);
                            f4 dw = zero;
#pragma unroll
                            for (int i = 0; i < 4; ++i) dw = mfma4(dt_[i], h_t[i], dw);  // D[o][k]
                            gadd(wl.g2(net, mo, ui), dw);
                        }
                        const f4 wb = tgrp(wl.g2(net, mo, ui));
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc = mfma4(wb[j], dlt[net][mo][j], acc);
                    }
                    dprev[net][ui] = acc * (4.f * rv * (1.f - rv));
                }
            }
#pragma unroll
            for (int lev = kMafLMax - 1; lev >= 1; --lev) {  // hidden layers L-1 .. 1
                if (lev < L) {
                    f4 dnext[2][UT];
#pragma unroll
                    for (int net = 0; net < 2; ++net) {
#pragma unroll
                        for (int ui = 0; ui < UT; ++ui) {
                            const f4 rv = level_r(lev - 1, net, ui);
                            f4 h_t = zero;
                            if (WG) h_t = transpose_tile(1.f - 2.f * rv, scrB, lane);
                            f4 acc = zero;
#pragma unroll
                            for (int uo = 0; uo < UT; ++uo) {
                                if (WG) {
                                    const f4 dt_ = transpose_tile(dprev[net][uo], scrA, lane);
                                    f4 dw = zero;
#pragma unroll
                                    for (int i = 0; i < 4; ++i) dw = mfma4(dt_[i], h_t[i], dw);
                                    gadd(wl.gh(lev - 1, net, uo, ui), dw);
                                }
                                const f4 wb = tgrp(wl.gh(lev - 1, net, uo, ui));
#pragma unroll
                                for (int j = 0; j < 4; ++j) acc = mfma4(wb[j], dprev[net][uo][j], acc);
                            }
                            dnext[net][ui] = acc * (4.f * rv * (1.f - rv));
                        }
                    }
#pragma unroll
                    for (int net = 0; net < 2; ++net)
#pragma unroll
                        for (int u = 0; u < UT; ++u) dprev[net][u] = dnext[net][u];
                }
            }
#pragma unroll
            for (int mm = 0; mm < DT; ++mm) {  // layer 0: inputs = x; a sweep wants N(v), the last pass dW only
                f4 x_t = zero;
                if (WG) x_t = transpose_tile(x[mm], scrB, lane);
                f4 acc = zero;
#pragma unroll
                for (int net = 0; net < 2; ++net) {
#pragma unroll
                    for (int ut = 0; ut < UT; ++ut) {
                        if (WG) {
                            const f4 dt_ = transpose_tile(dprev[net][ut], scrA, lane);
                            f4 dw = zero;
#pragma unroll
                            for (int i = 0; i < 4; ++i) dw = mfma4(dt_[i], x_t[i], dw);
                            gadd(wl.g0(net, ut, mm), dw);
                        } else {
                            const f4 wb = tgrp(wl.g0(net, ut, mm));
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc = mfma4(wb[j], dprev[net][ut][j], acc);
                        }
                    }
                }
                nv[mm] = acc;
            }
        };

        // ---- 2. D - 1 delta-only sweeps ----
        for (int sweep = 1; sweep < D; ++sweep) {
            // the transposed image and tanh' = 4 r (1 - r) are loop-invariant: with one hidden tile they may stay in
            // registers across the sweeps; with more, hoisting them out of the loop spills, so wider nets read the image
            // from LDS and rebuild tanh' (two VALU operations per element) in every sweep
            if (UT > 1) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int l = 0; l < kMafLMax; ++l)
#pragma unroll
                    for (int net = 0; net < 2; ++net)
#pragma unroll
                        for (int t = 0; t < UT; ++t)
                            if (l < L) asm volatile("" : "+v"(r[l][net][t]));
            }
            back(std::false_type{});
#pragma unroll
            for (int mm = 0; mm < DT; ++mm) v[mm] = ea[mm] * (g[mm] - nv[mm]);
        }
        // ---- 3. the last pass: weight gradients at (x; v, -g_ld) ----
        back(std::true_type{});
        if (row_ok && gob) {
#pragma unroll
            for (int mm = 0; mm < DT; ++mm) {
                const int f0 = 16 * mm + 4 * q;
                if (VEC) {
                    if (f0 < D) *reinterpret_cast<f4*>(gob + row * D + f0) = v[mm];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (f0 + j < D) gob[row * D + f0 + j] = v[mm][j];
                }
            }
        }
    }

    if (fusedm) {  // fold sums: 16 sample lanes -> this wave's LDS row -> the four rows in wave order -> global
        float* redw = red + wave * (2 * D + 1);
#pragma unroll
        for (int mm = 0; mm < DT; ++mm)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float va = fGZ[mm][j], vb = fGB[mm][j];
                for (int off = 8; off > 0; off >>= 1) {
                    va += __shfl_xor(va, off);
                    vb += __shfl_xor(vb, off);
                }
                const int f = 16 * mm + 4 * q + j;
                if (s == 0 && f < D) {
                    redw[f] = va;
                    redw[D + f] = vb;
                }
            }
        for (int off = 8; off > 0; off >>= 1) gs_acc += __shfl_xor(gs_acc, off);
        if (lane == 0) redw[2 * D] = gs_acc;
        __syncthreads();
        const bool own_row = a.Mp > 1 && gridDim.x == 1;
        float* gsum = a.g_sums + mp * (2 * D + 1);
        for (int i = threadIdx.x; i < 2 * D + 1; i += 256) {
            const int w = 2 * D + 1;
            const float v = ((red[i] + red[w + i]) + red[2 * w + i]) + red[3 * w + i];
            if (own_row) gsum[i] = v;
            else atomicAdd(gsum + i, v);
        }
    }
    __syncthreads();
    maf_bwd_flush<DT, UT, true>(gacc, nacc, wl, a.g_params + mp * a.gpstride, a.masks, D, U, a.Mp > 1 && gridDim.x == 1, lane,
                                wave);
}

// z = e^a (x - m) / alpha_bn + b,  sum_log_det = A(x) - sum log alpha_bn + sum a:
//   g_a = GZ - b GB + GS,  g_b = GB, added to the Affine slice of the gradient row (the only writer of that slice)
__global__ void __launch_bounds__(64)
ar_sample_fold_backward_kernel(const float* __restrict__ params, int64_t pstride, int64_t p_maf,
                               const float* __restrict__ g_sums, float* __restrict__ g_params, int64_t gpstride, int D) {
    const int64_t m = blockIdx.x;
    const float* ap = params + m * pstride + p_maf;
    float* gp = g_params + m * gpstride + p_maf;
    const float* gs = g_sums + m * (2 * D + 1);
    for (int d = threadIdx.x; d < D; d += 64) {
        gp[d] += gs[d] - ap[D + d] * gs[D + d] + gs[2 * D];
        gp[D + d] += gs[D + d];
    }
}

static std::atomic<long long> g_arsample_launches;

// The VEC instantiation moves x, g_x and g_omega as float4: D % 4 == 0 keeps every row a multiple of 16 bytes, so the
// rows are aligned exactly when the bases are.  (The sibling launch_maf_bwd_args of maf_bwd_mfma.hip still picks VEC on
// D % 4 == 0 alone and relies on 16-byte aligned tensors from its callers.)
static bool maf_sample_bwd_vec(const MafSampleBwdArgs& a) {
    return (a.D % 4) == 0 && is_aligned(a.x, 16) && (!a.g_x || is_aligned(a.g_x, 16)) && (!a.g_omega || is_aligned(a.g_omega, 16));
}

static int launch_maf_sample_bwd(MafSampleBwdArgs& a, hipStream_t st) {
    const MafBLayout wl = maf_blayout(a.D, a.L, a.U);
    a.nacc = maf_bwd_nacc(a.D, a.L, a.U);
    const size_t smem = maf_bwd_smem(wl, a.nacc);
    const dim3 grid = maf_bwd_grid(a.M, a.Mp, a.N);
    auto go = [&](auto dt) {  // D <= 32: one or two feature tiles
        return dispatch_1to4(wl.UT, [&](auto ut) {
            return dispatch_bool(maf_sample_bwd_vec(a), [&](auto vec) {
                return launch_lds("maf_sample_bwd", maf_sample_bwd_kernel<dt(), ut(), vec()>, grid, dim3(256), smem, st, a, wl);
            });
        });
    };
    return wl.DT == 1 ? go(int_c<1>{}) : go(int_c<2>{});
}

// workspace of tnf_ar_flow_sample_bwd_f32, described once: fold (Mp, 2, D) | ldc (Mp) | fold sums (Mp, 2 D + 1)
struct ArSampleWs {
    float *fold, *ldc, *g_sums;
    int64_t sums_bytes, bytes;
};
static ArSampleWs ar_sample_ws(int64_t Mp, int D, void* ws) {
    Carver c(ws);
    ArSampleWs w = {};
    w.fold = c.take<float>(Mp * 2 * D, 16);
    w.ldc = c.take<float>(Mp, 4);
    w.g_sums = c.take<float>(Mp * (2 * D + 1), 4);
    w.sums_bytes = Mp * (2 * D + 1) * (int64_t)sizeof(float);
    w.bytes = c.bytes(16);
    return w;
}

// the refusals the two calls share; TNF_OK: the shape runs
static int arsample_check(const char* fn, int64_t M, int64_t M_p, int64_t N, int D, int L, int U, int64_t need,
                          int64_t pstride, int64_t gpstride, const void* params, const void* g_params) {
    if (M < 1 || (M_p != 1 && M_p != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M=%lld M_p=%lld N=%lld", fn, (long long)M, (long long)M_p, (long long)N);
    if (!maf_bwd_mfma_supported(D, L, U)) return fail(TNF_EUNSUPPORTED, "%s: no kernel for D=%d L=%d U=%d", fn, D, L, U);
    if (pstride < need || gpstride < need)
        return fail(TNF_EINVAL, "%s: parameter rows shorter than %lld", fn, (long long)need);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_maf_sample_bwd_supported(int32_t D, int32_t L, int32_t U) { return maf_bwd_mfma_supported(D, L, U) ? 1 : 0; }

int64_t tnf_arsample_launch_count(void) { return g_arsample_launches.load(std::memory_order_relaxed); }

int tnf_maf_sample_bwd_f32(const float* x, const float* params, const float* masks, const float* g_x, const float* g_ld,
                           float* g_omega, float* g_params, int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t L,
                           int32_t U, int64_t pstride, int64_t gpstride, void* stream) {
    const char* fn = "tnf_maf_sample_bwd_f32";
    if (!x || !params || !masks || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_x && !g_ld) return fail(TNF_EINVAL, "%s: g_x and g_ld are both NULL", fn);
    if (int rc = arsample_check(fn, M, M_p, N, D, L, U, tnf_maf_num_params(D, L, U), pstride, gpstride, params, g_params))
        return rc;
    if (N == 0) return TNF_OK;
    MafSampleBwdArgs a = {};
    a.x = x; a.params = params; a.masks = masks; a.g_x = g_x; a.g_ld = g_ld; a.g_omega = g_omega; a.g_params = g_params;
    a.M = M; a.Mp = M_p; a.N = N; a.pstride = pstride; a.gpstride = gpstride; a.D = D; a.L = L; a.U = U;
    if (int rc = launch_maf_sample_bwd(a, as_stream(stream))) return rc;
    if (int rc = check_launch(fn)) return rc;
    g_arsample_launches.fetch_add(1, std::memory_order_relaxed);
    return TNF_OK;
}

int64_t tnf_ar_flow_sample_bwd_workspace_bytes(int64_t M_p, int32_t D) {
    if (M_p < 1 || D < 1)
        return fail(TNF_EINVAL, "tnf_ar_flow_sample_bwd_workspace_bytes: M_p=%lld D=%d", (long long)M_p, D);
    return ar_sample_ws(M_p, D, nullptr).bytes;
}

int tnf_ar_flow_sample_bwd_f32(const float* z, const float* params, const float* masks, const float* bn_mean,
                               const float* bn_alpha, const float* g_z, const float* g_sld, float* g_params, int64_t M,
                               int64_t M_p, int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_ar_flow_sample_bwd_f32";
    if (!z || !params || !masks || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: g_z and g_sld are both NULL", fn);
    const int64_t p_maf = tnf_maf_num_params(D, L, U);
    if (int rc = arsample_check(fn, M, M_p, N, D, L, U, p_maf + 2 * (int64_t)D, pstride, gpstride, params, g_params)) return rc;
    const ArSampleWs w = ar_sample_ws(M_p, D, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes)) return rc;
    if (!is_aligned(workspace, 16)) return fail(TNF_EINVAL, "%s: the workspace must be 16-byte aligned", fn);
    if (N == 0) return TNF_OK;
    hipStream_t st = as_stream(stream);
    if (int rc = launch_ar_fold(params, pstride, p_maf, bn_mean, bn_alpha, w.fold, w.ldc, M_p, D, 1, st)) return rc;
    if (hipMemsetAsync(w.g_sums, 0, (size_t)w.sums_bytes, st) != hipSuccess) return fail(TNF_ELAUNCH, "%s: memset failed", fn);
    MafSampleBwdArgs a = {};
    a.x = z; a.params = params; a.masks = masks; a.g_x = g_z; a.g_ld = g_sld; a.g_params = g_params;
    a.M = M; a.Mp = M_p; a.N = N; a.pstride = pstride; a.gpstride = gpstride; a.D = D; a.L = L; a.U = U;
    a.fold = w.fold; a.g_sums = w.g_sums;
    if (int rc = launch_maf_sample_bwd(a, st)) return rc;
    hipLaunchKernelGGL(ar_sample_fold_backward_kernel, dim3((unsigned)M_p), dim3(64), 0, st, params, pstride, p_maf,
                       (const float*)w.g_sums, g_params, gpstride, D);
    if (int rc = check_launch(fn)) return rc;
    g_arsample_launches.fetch_add(1, std::memory_order_relaxed);
    return TNF_OK;
}

}  // extern "C"
