// The body of the sampling backward walk (maf_sample_bwd.hip), included once per mode under its own kernel symbol:
//   MAF_SAMPLE_BWD_KERNEL  the kernel's name
//   MAF_SAMPLE_BWD_BATCH   false: tnf_arsample.h (rows x, or z with frozen statistics when fold != NULL)
//                          true:  tnf_arbatch.h (the stack with fresh batch statistics): fold holds five rows per
//                          parameter row, A' | B' | C0 | C1 | C2; the load stage rebuilds x = z A' + B' and forms
//                          g_x = g_z C0 + C1 + z C2 (the Affine and batch-statistics BatchNorm backward in closed form);
//                          the fold sums are not taken (ar_flow_batch.hip reduces them)
// Text inclusion, not a template parameter or a shared device function: either changed the machine code of the sixteen
// instantiations of the first mode.  No include guard on purpose.
template <int DT, int UT, bool VEC>
__global__ void __launch_bounds__(256)
MAF_SAMPLE_BWD_KERNEL(MafSampleBwdArgs a, MafBLayout wl) {
    constexpr bool BATCH = MAF_SAMPLE_BWD_BATCH;
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
    const bool fusedm = !BATCH && a.fold != nullptr;
    float* red = cst + 2 * D;
    if (fusedm)
        for (int i = threadIdx.x; i < 2 * D; i += 256) cst[i] = a.fold[mp * 2 * D + i];
    if (BATCH)
        for (int i = threadIdx.x; i < 5 * D; i += 256) cst[i] = a.fold[mp * 5 * D + i];
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
        if (BATCH) {  // the bijectors behind the MAF, statistics of the batch: x and g_x from z and g_z
#pragma unroll
            for (int mm = 0; mm < DT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mm + 4 * q + j;
                    if (f < D) {  // (padded features: x = g = 0 already; padded rows carry no cotangent)
                        const float zv = x[mm][j];
                        x[mm][j] = __builtin_fmaf(zv, cst[f], cst[D + f]);
                        const float gx = __builtin_fmaf(g[mm][j], cst[2 * D + f], __builtin_fmaf(zv, cst[4 * D + f], cst[3 * D + f]));
                        g[mm][j] = row_ok ? gx : 0.f;
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
