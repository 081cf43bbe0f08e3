// Per-context coupling flows with few samples per context (include/tnf_ctxflow.h): one parameter row per context m,
// 1 <= N <= 31 rows of z per context, the whole flow in ONE launch at every 2 <= D <= 64.
//
// Mapping.  One wave serves one context; a workgroup is CTX_WAVES such waves that share nothing (each has its own slice
// of the workgroup's LDS; no barrier).  The wave loads its context's rows once into the fp32 tile layout of mfma_tile.h
// -- NT tiles of 16 samples (NT = 1 for N <= 16, else 2), the two halves of a row in H-wide register tiles (H = 16 for
// D <= 32, 32 above) -- and walks the 2S coupling layers in the call's direction.  For each layer it copies the layer's
// block of the context's packed parameter row into its LDS slice with 16-byte loads (stage_block: the row leaves HBM as
// whole cache lines), gathers the exact-f32 MFMA operands from there (load_layer_w with the layer's real widths:
// h = D / 2 and D - h, bijectors.py:163-165, 250-254), runs coupling_tile on them from registers (RegOperands), and
// applies the BatchNorm / Affine maps between layers in registers from the shared (2S, D) statistics and the row's own
// Affine block.  Operands live in registers one layer at a time, so S is unbounded; there is no prepared image, no
// workspace and no second launch: a parameter row leaves HBM once (82 KB per context at D = 64, S = 4; 5 KB at D = 4,
// S = 1) and each z row is read once.
//
// Padding is exact.  A half narrower than H has zeros in its upper slots.  load_layer_w zero-fills the first layer's
// weight rows beyond the real conditioner width and the output layer's weight columns and biases beyond the real
// transformed width, so a padded conditioner slot multiplies a zero weight and a padded output slot gets t = 0, s = 0:
// (0 - 0) * 2^-0 = 0 inverse, 0 * 2^0 + 0 = 0 forward, and adds 0 to the log-det.  The map between layers uses
// (A, B) = (1, 0) there and no log-det term.  The padding therefore stays exactly 0 through every layer and the real
// slots see the arithmetic of the flow of width D.
#include <atomic>

#include "launch.h"
#include "mfma_tile.h"
#include "../../include/tnf_ctxflow.h"

namespace tnf {

constexpr int CTX_WAVES = 4;  // contexts per workgroup: one wave each, one per SIMD of the CU it lands on

static std::atomic<long long> g_ctxflow_launches[TNF_CTXFLOW_COUNTERS];

struct CtxFlowArgs {
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

// The parameter-only bijectors around coupling layer c, on the lane's slots of both halves (coupling_mfma.hip,
// fold_consts):  inverse: [Affine^-1 (c odd)] then BN^-1[c] before the layer,  v -> v (alpha / e^a) + (mu - shift alpha / e^a)
//                forward: BN[c] then [Affine (c odd)] after the layer,          v -> v (e^a / alpha) + (shift - mu e^a / alpha)
// asum += the Affine log-det terms a of the lane's real slots (the BatchNorm terms are summed once per wave, below).
template <int H, bool INV, int NT>
__device__ __forceinline__ void ctx_fold(const float* __restrict__ mean, const float* __restrict__ alpha,
                                         const float* __restrict__ ap, bool affine, int D, int q,
                                         f4 (&lo)[NT][(H + 15) / 16], f4 (&hi)[NT][(H + 15) / 16], float& asum) {
    constexpr int HT = (H + 15) / 16;
    const int h = D / 2;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int width = half ? D - h : h, base = half ? h : 0;
#pragma unroll
        for (int mm = 0; mm < HT; ++mm)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = 16 * mm + 4 * q + j;
                const bool ok = f < width;
                const int d = base + f;
                const float al = ok ? ld_sel(alpha, d, ok) : 1.f;
                const float mu = ld_sel(mean, d, ok);
                // e^(-a) inverse, e^a forward, in the hardware forms the tile itself uses (v_exp_f32, v_rcp_f32): the
                // kernel is bound by its vector instructions, and an IEEE division is ten of them per slot
                float es = 1.f, shift = 0.f;
                if (affine) {  // wave-uniform
                    const float av = ld_sel(ap, d, ok);
                    asum += av;
                    es = fast_exp(INV ? -av : av);
                    shift = ld_sel(ap + D, d, ok);
                }
                float A, B;
                if (INV) {
                    A = al * es;
                    B = mu - shift * A;
                } else {
                    A = es * __builtin_amdgcn_rcpf(al);
                    B = shift - mu * A;
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (half)
                        hi[t][mm][j] = __builtin_fmaf(hi[t][mm][j], A, B);
                    else
                        lo[t][mm][j] = __builtin_fmaf(lo[t][mm][j], A, B);
                }
            }
    }
}

// One contiguous block of a parameter row -> the wave's LDS buffer, as 16-byte loads: the ~100 strided dword gathers of
// load_layer_w then read LDS, and the row leaves HBM as whole cache lines (a dozen wide loads per lane and layer instead
// of a hundred narrow ones).  Rows need 4-byte alignment only: the copy runs over the 16-byte chunks that cover
// [src, src + n), and the first and the last chunk are read element by element, so nothing outside the block is touched.
// Returns where src[0] lies in the buffer.  One wave writes and reads its own buffer in program order: no barrier.
__device__ __forceinline__ const float* stage_block(float* buf, const float* __restrict__ src, int n, int lane) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const int head = (int)((a & 15) >> 2);  // floats of the first chunk that precede src
    const f4* g = reinterpret_cast<const f4*>(a & ~(uintptr_t)15);
    const int chunks = (head + n + 3) >> 2;
    for (int i = lane; i < chunks; i += 64) {
        f4 v;
        if (i == 0 || i == chunks - 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int idx = 4 * i + e - head;
                v[e] = ld_sel(src, idx, idx >= 0 && idx < n);
            }
        } else {
            v = g[i];
        }
        reinterpret_cast<f4*>(buf)[i] = v;
    }
    return buf + head;
}

// floats of the largest block staged at once: the lower coupling layer with the Affine block behind it, at U = 16, and
// the chunks' slack
template <int H, int L>
constexpr int ctx_stage_floats() {
    return 2 * (2 * H * 16 + H + 16 + (L - 1) * 17 * 16) + 4 * H + 8;
}

// The lane index as a value the optimiser cannot trace across a layer.  The gather indices of load_layer_w and the slot
// indices of ctx_fold depend on the lane and the shape only, so inside the stage loop they are loop invariants; hoisted,
// the ~100 indices and predicates per layer pair stay live across the whole loop and the kernel spills.  Recomputing them
// per layer is a few dozen integer instructions.  `after`: a value of the previous layer's result, which ties the gather
// behind that layer's arithmetic -- otherwise the scheduler starts the next layer's ~100 loads under the current layer
// and two layers' operands are live at once.  The latency of the gather is covered by the other waves of the SIMD.
// (An empty asm: no instruction is emitted.)
__device__ __forceinline__ int per_layer(int lane, float after) {
    asm volatile("" : "+v"(lane) : "v"(after));
    return lane;
}

template <int H, int L, bool INV, int NT>
__global__ void __launch_bounds__(CTX_WAVES * 64) __attribute__((amdgpu_waves_per_eu(H == 32 ? 2 : 3)))
ctx_flow_kernel(CtxFlowArgs a) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    constexpr int HT = (H + 15) / 16;
    // the wave index as a scalar: the context's base pointers then live in SGPRs and every gather is base + lane offset
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int64_t m = (int64_t)blockIdx.x * CTX_WAVES + wave;
    if (m >= a.M) return;  // whole waves leave: nothing below synchronises across waves
    const int D = a.D, N = a.N, U = a.U, h = D / 2, hh = D - h;
    const float* p = a.params + m * a.pstride;
    const FlowLayout fl = flow_layout(D, a.S, L, U);
    __shared__ __attribute__((aligned(16))) float stage[CTX_WAVES][ctx_stage_floats<H, L>()];
    float* buf = stage[wave];
    const int n_up = (int)fl.p_up, n_low = (int)fl.p_low + 2 * D;  // [upper layer] and [lower layer | Affine]

    // the context's rows, once: lane (s, q) holds slots 16 mm + 4 q + j of both halves of row 16 t + s
    f4 lo[NT][HT], hi[NT][HT];
    float ssum[NT];
    {
        const float* zb = a.z + (a.Mz == 1 ? 0 : m) * (int64_t)N * D;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int row = 16 * t + s;
            if (row >= N) row = N - 1;  // a copy of the last row: computed, never stored
            const float* zr = zb + (int64_t)row * D;
            ssum[t] = 0.f;
#pragma unroll
            for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mm + 4 * q + j;
                    lo[t][mm][j] = ld_sel(zr, f, f < h);
                    hi[t][mm][j] = ld_sel(zr + h, f, f < hh);
                }
        }
    }

    // BatchNorm's log-det, -sum log alpha over the (2S, D) statistics (bijectors.py:417): the same for every context,
    // summed by the wave while its row loads are in flight
    float ldc = 0.f;
    for (int i = lane; i < 2 * a.S * D; i += 64) ldc -= logf(a.bn_alpha[i]);
    ldc = wave_sum(ldc);
    float asum = 0.f;  // the Affine log-det terms of this lane's slots

    LayerW<H, L> w;
    if (INV) {
        // density_estimator.py:395-405: walk the stack backwards
        for (int st = a.S - 1; st >= 0; --st) {
            const float* ps = p + st * fl.stage;
            const int c1 = 2 * st + 1, c0 = 2 * st;
            const float* pl = stage_block(buf, ps + fl.p_up, n_low, per_layer(lane, ssum[0]));
            ctx_fold<H, true, NT>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, pl + fl.p_low, true, D, per_layer(lane, ssum[0]) >> 4, lo, hi, asum);
            load_layer_w<H, L>(w, pl, U, per_layer(lane, ssum[0]), hh, h);
            coupling_tile<H, L, true, NT>(RegOperands<H, L>{w}, hi, lo, ssum);
            const float* pu = stage_block(buf, ps, n_up, per_layer(lane, ssum[0]));
            ctx_fold<H, true, NT>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, pu, false, D, per_layer(lane, ssum[0]) >> 4, lo, hi, asum);
            load_layer_w<H, L>(w, pu, U, per_layer(lane, ssum[0]), h, hh);
            coupling_tile<H, L, true, NT>(RegOperands<H, L>{w}, lo, hi, ssum);
        }
    } else {
        // density_estimator.py:375-387
        for (int st = 0; st < a.S; ++st) {
            const float* ps = p + st * fl.stage;
            const int c0 = 2 * st, c1 = 2 * st + 1;
            const float* pu = stage_block(buf, ps, n_up, per_layer(lane, ssum[0]));
            load_layer_w<H, L>(w, pu, U, per_layer(lane, ssum[0]), h, hh);
            coupling_tile<H, L, false, NT>(RegOperands<H, L>{w}, lo, hi, ssum);
            ctx_fold<H, false, NT>(a.bn_mean + c0 * D, a.bn_alpha + c0 * D, pu, false, D, per_layer(lane, ssum[0]) >> 4, lo, hi, asum);
            const float* pl = stage_block(buf, ps + fl.p_up, n_low, per_layer(lane, ssum[0]));
            load_layer_w<H, L>(w, pl, U, per_layer(lane, ssum[0]), hh, h);
            coupling_tile<H, L, false, NT>(RegOperands<H, L>{w}, hi, lo, ssum);
            ctx_fold<H, false, NT>(a.bn_mean + c1 * D, a.bn_alpha + c1 * D, pl + fl.p_low, true, D, per_layer(lane, ssum[0]) >> 4, lo, hi, asum);
        }
    }
    ldc += reduce_q(asum);  // every lane of a q-group holds the same slots: the sum over q is the sum over the features

    float* zo = a.z_out ? a.z_out + m * (int64_t)N * D : nullptr;
    float* sldo = a.sum_log_det ? a.sum_log_det + m * (int64_t)N : nullptr;
    float* lpo = a.log_prob ? a.log_prob + m * (int64_t)N : nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int row = 16 * t + s;
        const bool row_ok = row < N;
        const float ld_tot = __builtin_fmaf(reduce_q(ssum[t]), kLn2, ldc);  // the tile code sums s * log2(e)
        if (INV && lpo) {
            float sq = 0.f;  // the padding is exactly 0: it adds nothing
#pragma unroll
            for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sq = __builtin_fmaf(lo[t][mm][j], lo[t][mm][j], sq);
                    sq = __builtin_fmaf(hi[t][mm][j], hi[t][mm][j], sq);
                }
            sq = reduce_q(sq);
            if (q == 0 && row_ok) lpo[row] = -0.5f * sq - (float)D * 0.91893853320467274178f - ld_tot;
        }
        if (sldo && q == 0 && row_ok) sldo[row] = ld_tot;
        if (zo && row_ok) {
            float* zr = zo + (int64_t)row * D;
#pragma unroll
            for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = 16 * mm + 4 * q + j;
                    if (f < h) zr[f] = lo[t][mm][j];
                    if (f < hh) zr[h + f] = hi[t][mm][j];
                }
        }
    }
}

static int launch_ctx_flow(const CtxFlowArgs& a, int L, bool inverse, int which, hipStream_t st) {
    const int64_t blocks = (a.M + CTX_WAVES - 1) / CTX_WAVES;
    g_ctxflow_launches[which].fetch_add(1, std::memory_order_relaxed);
    dispatch_1to3(L, [&](auto l) {
        return dispatch_bool(a.D > 32, [&](auto wide) {
            return dispatch_bool(inverse, [&](auto inv) {
                return dispatch_bool(a.N > 16, [&](auto two) {
                    constexpr int H = wide() ? 32 : 16, NT = two() ? 2 : 1;
                    hipLaunchKernelGGL((ctx_flow_kernel<H, l(), inv(), NT>), dim3((unsigned)blocks), dim3(CTX_WAVES * 64), 0,
                                       st, a);
                    return 0;
                });
            });
        });
    });
    return check_launch("ctx_flow");
}

// everything the two entries refuse before a launch, in the order of tnf_ctxflow.h (the NULL and output checks come first,
// with the callers)
static int ctxflow_checks(const char* fn, int64_t Mz, int64_t M, int64_t N, int D, int S, int L, int U, int64_t pstride) {
    if (M < 1 || (Mz != 1 && Mz != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M_z=%lld M=%lld N=%lld", fn, (long long)Mz, (long long)M, (long long)N);
    if (M > (int64_t)CTX_WAVES * 0x7fffffff) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!tnf_ctx_flow_supported(D, S, L, U, N == 0 ? 1 : N))
        return fail(TNF_EUNSUPPORTED, "%s: no per-context kernel for D=%d S=%d L=%d U=%d N=%lld", fn, D, S, L, U, (long long)N);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ctx_flow_supported(int32_t D, int32_t S, int32_t L, int32_t U, int64_t N) {
    return D >= 2 && D <= 64 && S >= 1 && L >= 1 && L <= 3 && U >= 1 && U <= 16 && N >= 1 && N <= 31 ? 1 : 0;
}

int64_t tnf_ctx_flow_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_CTXFLOW_COUNTERS) return fail(TNF_EINVAL, "tnf_ctx_flow_launch_count: counter %d", which);
    return g_ctxflow_launches[which].load(std::memory_order_relaxed);
}

int tnf_ctx_flow_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                              float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M, int64_t N, int32_t D,
                              int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_ctx_flow_log_prob_f32";
    if (!z || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!log_prob && !z0 && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = ctxflow_checks(fn, M_z, M, N, D, S, L, U, pstride)) return rc;
    if (z0 == z) return fail(TNF_EINVAL, "%s: z0 must not alias z", fn);
    if (N == 0) return TNF_OK;
    const CtxFlowArgs a{z, params, bn_mean, bn_alpha, z0, sum_log_det, log_prob, M_z, M, pstride, (int)N, D, S, U,
                        g_launch_gate};
    return launch_ctx_flow(a, L, true, TNF_CTXFLOW_COUNT_LOG_PROB, as_stream(stream));
}

int tnf_ctx_flow_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                             float* z_out, float* sum_log_det, int64_t M, int64_t N, int32_t D, int32_t S, int32_t L,
                             int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_ctx_flow_forward_f32";
    if (!omega || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!z_out && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = ctxflow_checks(fn, M, M, N, D, S, L, U, pstride)) return rc;
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    if (N == 0) return TNF_OK;
    const CtxFlowArgs a{omega, params, bn_mean, bn_alpha, z_out, sum_log_det, nullptr, M, M, pstride, (int)N, D, S, U,
                        g_launch_gate};
    return launch_ctx_flow(a, L, false, TNF_CTXFLOW_COUNT_FORWARD, as_stream(stream));
}

}  // extern "C"
