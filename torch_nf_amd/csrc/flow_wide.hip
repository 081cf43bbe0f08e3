// Whole-flow RealNVP kernel for hidden widths 17 <= U <= 64 at every 2 <= D <= 64 (include/tnf_wideflow.h): all 2S
// coupling layers, the BatchNorm / Affine maps between them and the base density in ONE launch, on the exact-f32 MFMA
// twin-MLP tile of coupling_wide.hip.
//
// Mapping.  One workgroup (WF_WAVES waves) owns one parameter row.  Prologue: all its waves build, straight from the
// packed row, the folded operand images of all 2S coupling layers in LDS (build_wide_image_io: real widths
// d_in / d_out per layer, zero-padded to 16 HT), and all its threads the per-layer fold constants (A, B) of the maps
// between layers (the arithmetic of fold_consts, coupling_mfma.hip); each wave sums the constant log-det
// sum(a) - sum(log alpha) for itself.  No prepared images, no workspace, no second launch; per-context rows work because
// the image is built per workgroup.  Tile loop: each wave walks 16-sample tiles.  It loads both halves of its rows once
// -- lane (s, q) holds slots 16 mm + 4 q + j of the lower half (features 0 .. h-1, h = D / 2) and of the upper half
// (features h .. D-1) of row s -- walks the layers last-to-first (inverse) or first-to-last (FWD) with the two register
// halves swapping the conditioner / transformed roles, applies the fold in registers between layers and writes its
// outputs once: z never round-trips through HBM between layers.
//
// Padding is exact.  A half narrower than 16 HT has zeros in its upper slots.  The image has
// zero weight rows beyond a layer's real input width and zero weight columns and biases beyond its real output width,
// so a padded conditioner slot multiplies a zero weight and a padded transformed slot gets t = 0, s = 0:
// (0 - 0) 2^-0 = 0 inverse, 0 2^0 + 0 = 0 forward, and adds 0 to the log-det.  The fold of a padded slot is (A, B) =
// (1, 0) with no log-det term.  The padding therefore stays exactly 0 through every layer, adds 0 to |z0|^2, and the
// real slots see the arithmetic of the flow of width D.
//
// Memory.  Rows of z need 4-byte alignment only: float4 loads / stores are used when the row base is 16-byte aligned and
// D % 8 == 0 (both half offsets are then multiples of 16 bytes), element accesses otherwise.  Nothing outside a row's D
// floats or a parameter row's tnf_flow_num_params floats is read or written; rows beyond N are clamped copies of the
// last row, computed and never stored.
//
// DEEP (L >= 4) takes the activation with a refined reciprocal (wide_flow_tile.h: sig2_nr).
// Per tile and layer 2 * 4 * (HT UT + (L-1) UT UT + HT UT) MFMAs (coupling_wide.hip); LDS per workgroup:
// wide_flow_tile.h.  With 50 .. 150 KB of images one workgroup per CU is all that fits, so the workgroup is 8 waves:
// two per SIMD, each with two independent accumulator chains (t-net, s-net), cover the dependent fp32-MFMA latency and
// the exp2 / rcp sections between layers.
#include <atomic>

#include "launch.h"
#include "wide_flow_tile.h"
#include "../../include/tnf_wideflow.h"

namespace tnf {

constexpr int WF_WAVES = 8;

static std::atomic<long long> g_wideflow_launches[TNF_WIDEFLOW_COUNTERS];

struct WideFlowArgs {
    const float* z;        // (Mz, N, D), Mz in {1, M}
    const float* params;   // (Mp, pstride), Mp in {1, M}
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    float* z_out;          // (M, N, D) or NULL
    float* sum_log_det;    // (M, N) or NULL
    float* log_prob;       // (M, N) or NULL (inverse only)
    int64_t Mz, Mp, N, pstride;
    int D, S, U;
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

template <int HT, int UT, bool FWD, bool DEEP>
__global__ void __launch_bounds__(WF_WAVES * 64)
flow_wide_kernel(WideFlowArgs a, WideLayout wl) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int64_t m = grid_m();
    const int64_t M = a.Mz > a.Mp ? a.Mz : a.Mp;
    if (m >= M) return;  // the whole workgroup leaves
    const int D = a.D, S = a.S, U = a.U, h = D / 2, hh = D - h;
    const float* p = a.params + (a.Mp == 1 ? 0 : m) * a.pstride;
    const FlowLayout fl = flow_layout(D, S, wl.L, U);
    const int img_floats = wl.floats(), layer_floats = img_floats + 64 * HT;  // [image | fold] per coupling layer

    // ---- prologue: the images and fold constants of all 2S layers ----
    {
        int unit = 0;
        for (int c = 0; c < 2 * S; ++c) {
            const int upper = (c & 1) == 0;  // RealNVP(upper) first (density_estimator.py:260-270)
            const float* pc = p + (c >> 1) * fl.stage + (upper ? 0 : fl.p_up);
            build_wide_image_io(lds + c * layer_floats, pc, wl, upper ? h : hh, upper ? hh : h, U, lane, wave, WF_WAVES, unit);
        }
        // fold slot (c, half, f): the feature d = (half ? h : 0) + f when f is inside the half, else (1, 0)
        for (int i = threadIdx.x; i < 2 * S * 32 * HT; i += WF_WAVES * 64) {
            const int c = i / (32 * HT), r = i - c * (32 * HT), half = r / (16 * HT), f = r - half * (16 * HT);
            float A = 1.f, B = 0.f;
            if (f < (half ? hh : h)) {
                const int d = (half ? h : 0) + f;
                const float alpha = a.bn_alpha[c * D + d], mu = a.bn_mean[c * D + d];
                float ea = 1.f, shift = 0.f;
                if (c & 1) {
                    const float* ap = p + (c >> 1) * fl.stage + fl.p_up + fl.p_low;
                    ea = expf(ap[d]);
                    shift = ap[D + d];
                }
                if (!FWD) {  // before layer c: Affine^-1 (c odd), then BN^-1[c]
                    A = alpha / ea;
                    B = mu - shift * A;
                } else {  // after layer c: BN[c], then Affine (c odd)
                    A = ea / alpha;
                    B = shift - mu * A;
                }
            }
            float* fold = lds + c * layer_floats + img_floats;
            fold[r] = A;
            fold[32 * HT + r] = B;
        }
    }
    // the parameter-only log-dets, sum(a) - sum(log alpha) (bijectors.py:293, 417): every wave sums them for itself, in
    // one order, so that all waves hold the same bits
    float ldc = 0.f;
    for (int i = lane; i < 2 * S * D; i += 64) {
        const int c = i / D, d = i - c * D;
        float ld = -logf(a.bn_alpha[i]);
        if (c & 1) ld += p[(c >> 1) * fl.stage + fl.p_up + fl.p_low + d];
        ldc += ld;
    }
    ldc = wave_sum(ldc);
    __syncthreads();

    const float* zb = a.z + (a.Mz == 1 ? 0 : m) * a.N * D;
    float* zo = a.z_out ? a.z_out + m * a.N * D : nullptr;
    float* sldo = a.sum_log_det ? a.sum_log_det + m * a.N : nullptr;
    float* lpo = a.log_prob ? a.log_prob + m * a.N : nullptr;
    // float4 accesses: a 16-byte aligned base and D % 8 == 0 make every row and both half offsets 16-byte aligned, and
    // every float4 of a half lies wholly inside or wholly outside it (h % 4 == 0)
    const bool vec_in = (D & 7) == 0 && (reinterpret_cast<uintptr_t>(zb) & 15) == 0;
    const bool vec_out = (D & 7) == 0 && (reinterpret_cast<uintptr_t>(zo) & 15) == 0;
    const f4 zero = {0.f, 0.f, 0.f, 0.f};

    const int64_t ntiles = (a.N + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.x * WF_WAVES + wave; tile < ntiles; tile += (int64_t)gridDim.x * WF_WAVES) {
        const int64_t row = tile * 16 + s;
        const bool row_ok = row < a.N;
        const float* zr = zb + (row_ok ? row : a.N - 1) * D;  // a copy of the last row: computed, never stored
        f4 lo[HT], hi[HT];
        if (vec_in) {
#pragma unroll
            for (int mm = 0; mm < HT; ++mm) {
                const int f = 16 * mm + 4 * q;
                lo[mm] = f < h ? *reinterpret_cast<const f4*>(zr + f) : zero;
                hi[mm] = f < h ? *reinterpret_cast<const f4*>(zr + h + f) : zero;
            }
        } else {
#pragma unroll
            for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mm + 4 * q + j;
                    lo[mm][j] = ld_sel(zr, f, f < h);
                    hi[mm][j] = ld_sel(zr + h, f, f < hh);
                }
        }
        asm volatile("" ::: "memory");  // operand reads stay inside the tile loop
        float ssum = 0.f;
        if (!FWD) {
            // density_estimator.py:395-405: walk the stack backwards
            for (int st = S - 1; st >= 0; --st) {
                const float* l1 = lds + (2 * st + 1) * layer_floats;
                const float* l0 = lds + (2 * st) * layer_floats;
                wide_flow_fold<HT>(l1 + img_floats, q, lo, hi);
                wide_flow_layer<HT, UT, true, DEEP>(l1, wl, lane, hi, lo, ssum);  // lower: conditioned on the upper half
                wide_flow_fold<HT>(l0 + img_floats, q, lo, hi);
                wide_flow_layer<HT, UT, true, DEEP>(l0, wl, lane, lo, hi, ssum);  // upper: conditioned on the lower half
            }
        } else {
            // density_estimator.py:375-387
            for (int st = 0; st < S; ++st) {
                const float* l0 = lds + (2 * st) * layer_floats;
                const float* l1 = lds + (2 * st + 1) * layer_floats;
                wide_flow_layer<HT, UT, false, DEEP>(l0, wl, lane, lo, hi, ssum);
                wide_flow_fold<HT>(l0 + img_floats, q, lo, hi);
                wide_flow_layer<HT, UT, false, DEEP>(l1, wl, lane, hi, lo, ssum);
                wide_flow_fold<HT>(l1 + img_floats, q, lo, hi);
            }
        }
        const float ld_tot = __builtin_fmaf(reduce_q(ssum), kLn2, ldc);  // the tile code sums s log2(e)
        if (!FWD && lpo) {
            float sq = 0.f;  // the padding is exactly 0: it adds nothing
#pragma unroll
            for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sq = __builtin_fmaf(lo[mm][j], lo[mm][j], sq);
                    sq = __builtin_fmaf(hi[mm][j], hi[mm][j], sq);
                }
            sq = reduce_q(sq);
            if (q == 0 && row_ok) lpo[row] = -0.5f * sq - (float)D * 0.91893853320467274178f - ld_tot;
        }
        if (sldo && q == 0 && row_ok) sldo[row] = ld_tot;
        if (zo && row_ok) {
            float* zw = zo + row * D;
            if (vec_out) {
#pragma unroll
                for (int mm = 0; mm < HT; ++mm) {
                    const int f = 16 * mm + 4 * q;
                    if (f < h) {
                        *reinterpret_cast<f4*>(zw + f) = lo[mm];
                        *reinterpret_cast<f4*>(zw + h + f) = hi[mm];
                    }
                }
            } else {
#pragma unroll
                for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int f = 16 * mm + 4 * q + j;
                        if (f < h) zw[f] = lo[mm][j];
                        if (f < hh) zw[h + f] = hi[mm][j];
                    }
            }
        }
    }
}

static int launch_wide_flow(const WideFlowArgs& a, int L, bool fwd, int which, hipStream_t st) {
    const WideLayout wl = wide_flow_layout(a.D, L, a.U);
    const size_t smem = (size_t)wide_flow_lds_bytes(a.D, a.S, L, a.U);
    const int64_t M = a.Mz > a.Mp ? a.Mz : a.Mp;
    const int64_t ntiles = (a.N + 15) / 16;
    // one workgroup per CU is all the LDS admits: one resident round of workgroups
    const dim3 grid = grid_xm(persistent_bx(ntiles, WF_WAVES, 256, M), M);
    g_wideflow_launches[which].fetch_add(1, std::memory_order_relaxed);
    const int rc = dispatch_bool(wl.HT > 1, [&](auto two) {
        return dispatch_range<2, 4>(wl.UT, [&](auto ut) {
            return dispatch_bool(fwd, [&](auto f) {
                return dispatch_bool(L > 3, [&](auto deep) {  // the refined activation of wide_flow_tile.h
                    constexpr int HT = two() ? 2 : 1;
                    return launch_lds("wide_flow", flow_wide_kernel<HT, ut(), f(), deep()>, grid, dim3(WF_WAVES * 64), smem,
                                      st, a, wl);
                });
            });
        });
    });
    if (rc != TNF_OK) return rc;
    return check_launch("wide_flow");
}

// everything the two entries refuse before a launch, in the order of tnf_wideflow.h (the NULL and output checks come
// first, with the callers)
static int wideflow_checks(const char* fn, int64_t Mz, int64_t Mp, int64_t N, int D, int S, int L, int U, int64_t pstride,
                           bool sampling) {
    const int64_t M = Mz > Mp ? Mz : Mp;
    if (Mz < 1 || Mp < 1 || (Mz != 1 && Mz != M) || (Mp != 1 && Mp != M) || (sampling && Mz != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M_z=%lld M_p=%lld N=%lld", fn, (long long)Mz, (long long)Mp, (long long)N);
    if (M > (int64_t)32768 * 65535) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!wide_flow_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no whole-flow wide kernel for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_wide_flow_supported(int32_t D, int32_t S, int32_t L, int32_t U) { return wide_flow_supported(D, S, L, U) ? 1 : 0; }

int64_t tnf_wide_flow_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_WIDEFLOW_COUNTERS) return fail(TNF_EINVAL, "tnf_wide_flow_launch_count: counter %d", which);
    return g_wideflow_launches[which].load(std::memory_order_relaxed);
}

int tnf_wide_flow_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                               float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N,
                               int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_wide_flow_log_prob_f32";
    if (!z || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!log_prob && !z0 && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = wideflow_checks(fn, M_z, M_p, N, D, S, L, U, pstride, false)) return rc;
    if (z0 == z) return fail(TNF_EINVAL, "%s: z0 must not alias z", fn);
    if (N == 0) return TNF_OK;
    const WideFlowArgs a{z, params, bn_mean, bn_alpha, z0, sum_log_det, log_prob, M_z, M_p, N, pstride, D, S, U,
                         g_launch_gate};
    return launch_wide_flow(a, L, false, TNF_WIDEFLOW_COUNT_LOG_PROB, as_stream(stream));
}

int tnf_wide_flow_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* z_out, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N, int32_t D, int32_t S,
                              int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_wide_flow_forward_f32";
    if (!omega || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!z_out && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = wideflow_checks(fn, M_z, M_p, N, D, S, L, U, pstride, true)) return rc;
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    if (N == 0) return TNF_OK;
    const WideFlowArgs a{omega, params, bn_mean, bn_alpha, z_out, sum_log_det, nullptr, M_z, M_p, N, pstride, D, S, U,
                         g_launch_gate};
    return launch_wide_flow(a, L, true, TNF_WIDEFLOW_COUNT_FORWARD, as_stream(stream));
}

}  // extern "C"
