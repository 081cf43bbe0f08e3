// Per-context coupling flows with 17 <= U <= 64 hidden units and few samples per context (include/tnf_ctxwide.h): one
// parameter row per context m, 1 <= N <= 31 rows of z per context, the whole flow in ONE launch at every 2 <= D <= 64
// and any S.  flow_ctx.hip serves this layout up to 16 units; flow_wide.hip serves these widths with the images of all
// 2S layers resident, which bounds S by LDS and leaves its eight waves on at most two tiles here.
//
// Mapping.  One workgroup (cw_waves<UT>() waves: 2 or 4) serves one context.  Wave t < NT holds the context's tile t (16 samples;
// NT = 1 for N <= 16, else 2) in registers for the whole flow: lane (s, q) holds slots 16 mm + 4 q + j of the lower and
// of the upper half of row 16 t + s, as in flow_wide.hip.  The workgroup walks the 2S coupling layers in the call's
// direction ONE LAYER AT A TIME.  Per layer: all waves build the layer's folded exact-f32 operand image in LDS straight
// from the context's packed row (build_wide_image_io: the image's (net, 16 output units) blocks are dealt over the
// waves) and all threads the layer's fold block [A_lo | A_hi | B_lo | B_hi] from the shared (2S, D) statistics and the
// row's Affine block (the arithmetic of flow_wide.hip's prologue); barrier; the tile-holding waves run wide_flow_layer
// and wide_flow_fold on their registers; barrier; the next layer's image overwrites this one.  One image and one fold
// block are resident (ctx_wide.h: 17 KB at D = 4, U = 20, L = 2; 150 KB at D <= 32, U = 64, L = 5), so S is unbounded.
// No prepared image, no workspace, no second launch; a parameter row leaves HBM once and each z row is read once.
//
// Padding is exact by the argument of flow_wide.hip: zero weight rows beyond a layer's real input
// width, zero weight columns and biases beyond its real output width and a fold of (1, 0) keep every padded slot at
// exactly 0 through every layer; it adds 0 to the log-det and to |z0|^2.  Rows beyond N are clamped copies of the last
// row: computed, never stored.  Rows need 4-byte alignment only (element accesses); nothing outside a row's D floats or
// a parameter row's tnf_flow_num_params floats is read or written.  DEEP (L >= 4): the activation with the refined
// reciprocal (wide_flow_tile.h: sig2_nr).
#include <atomic>

#include "ctx_wide.h"
#include "../../include/tnf_ctxwide.h"

namespace tnf {

// Waves per workgroup: one or two hold a tile, all build the images.  Measured at 2, 4 and 8 (DESIGN.md 25.6,
// profiles/r22_ctxwidebench_waves.txt): up to 32 units (UT = 2) two waves are 1.02 .. 1.3 x faster than four -- the image
// is 17 .. 35 KB, several workgroups share a CU, and a smaller workgroup has cheaper barriers and no idle wave at
// N > 16; at 64 units (UT = 4) four waves tie with two at D <= 32 and are 1.5 x faster at D = 64, where the 134 KB image
// leaves one workgroup per CU and its waves are all the gathers in flight; eight lose everywhere.  UT = 3 was not
// measured and takes four.
template <int UT>
constexpr int cw_waves() { return UT == 2 ? 2 : 4; }

std::atomic<long long> g_ctxwide_launches[TNF_CTXWIDE_COUNTERS];  // shared with flow_ctx_wide_bwd.hip

struct CtxWideArgs {
    const float* z;        // (Mz, N, D), Mz in {1, M}
    const float* params;   // (M, pstride)
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    float* z_out;          // (M, N, D) or NULL
    float* sum_log_det;    // (M, N) or NULL
    float* log_prob;       // (M, N) or NULL (inverse only)
    int64_t Mz, M, pstride;
    int N, D, S, U;
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

template <int HT, int UT, bool FWD, bool DEEP>
__global__ void __launch_bounds__(cw_waves<UT>() * 64)
ctx_wide_kernel(CtxWideArgs a, WideLayout wl) {
    constexpr int CW_WAVES = cw_waves<UT>();
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float cw_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int64_t m = grid_m();
    if (m >= a.M) return;  // the whole workgroup leaves
    const int D = a.D, N = a.N, S = a.S, U = a.U, h = D / 2, hh = D - h;
    const float* p = a.params + m * a.pstride;
    const FlowLayout fl = flow_layout(D, S, wl.L, U);
    float* img = cw_lds;
    float* fold = cw_lds + wl.floats();
    const bool holds = 16 * wave < N;  // wave-uniform: this wave holds tile `wave`
    const int row = 16 * wave + s;
    const bool row_ok = row < N;

    f4 lo[HT], hi[HT];
    float ldc = 0.f, ssum = 0.f;
    if (holds) {
        const float* zr = a.z + ((a.Mz == 1 ? 0 : m) * (int64_t)N + (row_ok ? row : N - 1)) * D;
#pragma unroll
        for (int mm = 0; mm < HT; ++mm)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * mm + 4 * q + j;
                lo[mm][j] = ld_sel(zr, f, f < h);
                hi[mm][j] = ld_sel(zr + h, f, f < hh);
            }
        // the parameter-only log-dets, sum(a) - sum(log alpha) (bijectors.py:293, 417): each tile-holding wave sums
        // them for itself, in one order, so that both hold the same bits
        for (int i = lane; i < 2 * S * D; i += 64) {
            const int c = i / D, d = i - c * D;
            float ld = -logf(a.bn_alpha[i]);
            if (c & 1) ld += p[(c >> 1) * fl.stage + fl.p_up + fl.p_low + d];
            ldc += ld;
        }
        ldc = wave_sum(ldc);
    } else {
#pragma unroll
        for (int mm = 0; mm < HT; ++mm) lo[mm] = hi[mm] = f4{0.f, 0.f, 0.f, 0.f};
    }

    for (int i = 0; i < 2 * S; ++i) {
        const int c = FWD ? i : 2 * S - 1 - i;  // density_estimator.py:375-387 forward, :395-405 backwards
        const int upper = (c & 1) == 0;         // RealNVP(upper) first (density_estimator.py:260-270)
        const float* ps = p + (c >> 1) * fl.stage;
        if (i) __syncthreads();  // the previous layer's operands have been read
        int unit = 0;
        build_wide_image_io(img, ps + (upper ? 0 : fl.p_up), wl, upper ? h : hh, upper ? hh : h, U, lane, wave, CW_WAVES, unit);
        // fold slot (half, f): the feature d = (half ? h : 0) + f when f is inside the half, else (1, 0)
        for (int r = threadIdx.x; r < 32 * HT; r += CW_WAVES * 64) {
            const int half = r / (16 * HT), f = r - half * (16 * HT);
            float A = 1.f, B = 0.f;
            if (f < (half ? hh : h)) {
                const int d = (half ? h : 0) + f;
                const float alpha = a.bn_alpha[c * D + d], mu = a.bn_mean[c * D + d];
                float ea = 1.f, shift = 0.f;
                if (c & 1) {
                    const float* ap = ps + fl.p_up + fl.p_low;
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
            fold[r] = A;
            fold[32 * HT + r] = B;
        }
        __syncthreads();
        if (holds) {
            if (!FWD) {
                wide_flow_fold<HT>(fold, q, lo, hi);
                if (upper) wide_flow_layer<HT, UT, true, DEEP>(img, wl, lane, lo, hi, ssum);  // conditioned on the lower half
                else wide_flow_layer<HT, UT, true, DEEP>(img, wl, lane, hi, lo, ssum);
            } else {
                if (upper) wide_flow_layer<HT, UT, false, DEEP>(img, wl, lane, lo, hi, ssum);
                else wide_flow_layer<HT, UT, false, DEEP>(img, wl, lane, hi, lo, ssum);
                wide_flow_fold<HT>(fold, q, lo, hi);
            }
        }
    }
    if (!holds) return;  // no barrier below

    const float ld_tot = __builtin_fmaf(reduce_q(ssum), kLn2, ldc);  // the tile code sums s log2(e)
    if (!FWD && a.log_prob) {
        float sq = 0.f;  // the padding is exactly 0: it adds nothing
#pragma unroll
        for (int mm = 0; mm < HT; ++mm)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sq = __builtin_fmaf(lo[mm][j], lo[mm][j], sq);
                sq = __builtin_fmaf(hi[mm][j], hi[mm][j], sq);
            }
        sq = reduce_q(sq);
        if (q == 0 && row_ok) a.log_prob[m * (int64_t)N + row] = -0.5f * sq - (float)D * 0.91893853320467274178f - ld_tot;
    }
    if (a.sum_log_det && q == 0 && row_ok) a.sum_log_det[m * (int64_t)N + row] = ld_tot;
    if (a.z_out && row_ok) {
        float* zw = a.z_out + (m * (int64_t)N + row) * D;
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

static int launch_ctx_wide(const CtxWideArgs& a, int L, bool fwd, int which, hipStream_t st) {
    const WideLayout wl = wide_flow_layout(a.D, L, a.U);
    const size_t smem = (size_t)ctx_wide_lds_bytes(0, a.D, a.S, L, a.U, a.N);
    const dim3 grid = grid_xm(1, a.M);
    g_ctxwide_launches[which].fetch_add(1, std::memory_order_relaxed);
    const int rc = dispatch_bool(wl.HT > 1, [&](auto two) {
        return dispatch_range<2, 4>(wl.UT, [&](auto ut) {
            return dispatch_bool(fwd, [&](auto f) {
                return dispatch_bool(L > 3, [&](auto deep) {  // the refined activation of wide_flow_tile.h
                    constexpr int HT = two() ? 2 : 1;
                    return launch_lds("ctx_wide", ctx_wide_kernel<HT, ut(), f(), deep()>, grid, dim3(cw_waves<ut()>() * 64), smem,
                                      st, a, wl);
                });
            });
        });
    });
    if (rc != TNF_OK) return rc;
    return check_launch("ctx_wide");
}

// everything the two entries refuse before a launch, in the order of tnf_ctxflow.h (the NULL and output checks come
// first, with the callers)
static int ctxwide_checks(const char* fn, int64_t Mz, int64_t M, int64_t N, int D, int S, int L, int U, int64_t pstride) {
    if (M < 1 || (Mz != 1 && Mz != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M_z=%lld M=%lld N=%lld", fn, (long long)Mz, (long long)M, (long long)N);
    if (M > (int64_t)32768 * 65535) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!ctx_wide_supported(D, S, L, U, N == 0 ? 1 : N))
        return fail(TNF_EUNSUPPORTED, "%s: no wide per-context kernel for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L, U,
                    (long long)N);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_wide_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return ctx_wide_supported(D, S, L, U, N) ? 1 : 0;
}

int tnf_ctx_wide_train_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return ctx_wide_train_supported(D, S, L, U, N) ? 1 : 0;
}

int64_t tnf_ctx_wide_lds_bytes(int32_t which, int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return ctx_wide_lds_bytes(which, D, S, L, U, N);
}

int64_t tnf_ctx_wide_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_CTXWIDE_COUNTERS) return fail(TNF_EINVAL, "tnf_ctx_wide_launch_count: counter %d", which);
    return g_ctxwide_launches[which].load(std::memory_order_relaxed);
}

int tnf_ctx_wide_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M, int64_t N, int32_t D,
                              int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_ctx_wide_log_prob_f32";
    if (!z || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!log_prob && !z0 && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = ctxwide_checks(fn, M_z, M, N, D, S, L, U, pstride)) return rc;
    if (z0 == z) return fail(TNF_EINVAL, "%s: z0 must not alias z", fn);
    if (N == 0) return TNF_OK;
    const CtxWideArgs a{z, params, bn_mean, bn_alpha, z0, sum_log_det, log_prob, M_z, M, pstride, (int)N, D, S, U,
                        g_launch_gate};
    return launch_ctx_wide(a, L, false, TNF_CTXWIDE_COUNT_LOG_PROB, as_stream(stream));
}

int tnf_ctx_wide_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                             float* z_out, float* sum_log_det, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L,
                             int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_ctx_wide_forward_f32";
    if (!omega || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!z_out && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = ctxwide_checks(fn, M, M, N, D, S, L, U, pstride)) return rc;
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    if (N == 0) return TNF_OK;
    const CtxWideArgs a{omega, params, bn_mean, bn_alpha, z_out, sum_log_det, nullptr, M, M, pstride, (int)N, D, S, U,
                        g_launch_gate};
    return launch_ctx_wide(a, L, true, TNF_CTXWIDE_COUNT_FORWARD, as_stream(stream));
}

}  // extern "C"
