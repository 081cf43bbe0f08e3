// Streamed whole-flow RealNVP kernel for hidden widths 17 <= U <= 64 at every 2 <= D <= 64 and ANY number of stages
// (include/tnf_widestream.h): all 2S coupling layers, the BatchNorm / Affine maps between them and the base density in
// ONE launch.  flow_wide.hip does this with the operand images of all 2S layers resident in LDS, which caps S at 4, 2, 1
// or 0 (wide_flow_supported); flow_ctx_wide.hip walks layer by layer with one image resident, for at most two tiles per
// parameter row.  This kernel is that walk for rows with many samples.
//
// Mapping.  One workgroup (WS_WAVES = 8 waves) serves one parameter row and walks GROUPS of 8 T tiles (128 T samples):
// wave w holds tiles 8 T g + 8 t + w, t < T, of group g in registers, in the lane layout of flow_wide.hip (lane (s, q):
// slots 16 mm + 4 q + j of the lower and of the upper half of row s).  For each group the workgroup walks the 2S layers
// in the call's direction; per layer every wave runs wide_flow_fold and wide_flow_layer (wide_flow_tile.h: the code of
// flow_wide.hip) on its tiles with operands from the layer's slot in LDS, and writes its outputs once at the end: z
// never round-trips through HBM between layers.  The group loop's trip count is the same for all waves of a workgroup.
//
// Image ring.  LDS holds one or two slots of wide_flow_layer_floats(D, L, U) floats, [image | fold block].  Walk
// position i (layer c = i forward, 2S-1-i inverse) lives in slot i & 1 (two slots) or slot 0 (one slot).
//   two slots: a wave that has finished position i on its tiles builds its share of position i + 1 into the other slot
//              (build_wide_image_io: the image's (net, 16 output units) blocks dealt over the waves; the fold block
//              with the arithmetic of flow_wide.hip's prologue), then ONE barrier.  The slot written at step i was last
//              read at step i - 1, whose barrier every wave has passed; it is read at step i + 1, after this barrier.
//              2S is even, so position 0 is slot 0 in every group and the ring runs on across groups: the last step of
//              a group builds position 0 of the next.
//   one slot:  compute, barrier (every read of the slot is over), build, barrier.
// The very last step of a workgroup builds nothing.  Every barrier is reached by all 512 threads the same number of
// times: the only exit before them (m >= M, the launch gate) is workgroup-uniform, waves whose tiles lie beyond the
// row's last tile skip the arithmetic only, and no per-wave condition encloses a barrier.
//
// Padding, memory, DEEP: exactly flow_wide.hip: padded slots stay 0; rows of z need 4-byte alignment,
// float4 accesses when the row base is 16-byte aligned and D % 8 == 0; rows beyond N are clamped copies of the last
// row, computed and never stored; nothing outside a row's D floats or a parameter row's tnf_flow_num_params floats is
// touched.  No workspace, no prepared images, no second launch, no atomics.  The constant log-det sum(a) - sum(log alpha)
// is summed per wave in flow_wide.hip's order, and a tile's arithmetic is flow_wide.hip's: the two kernels agree bit for
// bit where both apply.
#include <atomic>

#include "launch.h"
#include "wide_stream.h"
#include "../../include/tnf_widestream.h"

namespace tnf {

static std::atomic<long long> g_widestream_launches[TNF_WIDESTREAM_COUNTERS];
static std::atomic<int> g_widestream_tiles{0};  // 0: the rule; a shipped T: forced (tnf_wide_flow_stream_set_tiles)

struct WideStreamArgs {
    const float* z;        // (Mz, N, D), Mz in {1, M}
    const float* params;   // (Mp, pstride), Mp in {1, M}
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    float* z_out;          // (M, N, D) or NULL
    float* sum_log_det;    // (M, N) or NULL
    float* log_prob;       // (M, N) or NULL (inverse only)
    int64_t Mz, Mp, N, pstride;
    int D, S, U;
    int slots;             // 1 or 2 (wide_stream_slots)
    const int* gate;       // optional device flag: the kernel returns at once while *gate == 0 (tnf_set_launch_gate)
};

template <int HT, int UT, bool FWD, bool DEEP, int T>
__global__ void __launch_bounds__(WS_WAVES * 64)
flow_wide_stream_kernel(WideStreamArgs a, WideLayout wl) {
    if (a.gate && *a.gate == 0) return;  // a conditionally needed launch (tnf_set_launch_gate): nothing to do
    extern __shared__ __attribute__((aligned(16))) float ws_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = lane & 15, q = lane >> 4;
    const int64_t m = grid_m();
    const int64_t M = a.Mz > a.Mp ? a.Mz : a.Mp;
    if (m >= M) return;  // the whole workgroup leaves, before any barrier
    const int D = a.D, S = a.S, U = a.U, h = D / 2, hh = D - h;
    const float* p = a.params + (a.Mp == 1 ? 0 : m) * a.pstride;
    const FlowLayout fl = flow_layout(D, S, wl.L, U);
    const int img_floats = wl.floats(), layer_floats = img_floats + 64 * HT;  // [image | fold] per slot
    const bool two = a.slots == 2;

    // walk position i -> its layer's image and fold block into `slot`; all waves, no barrier inside
    auto build = [&](int i, float* slot) {
        const int c = FWD ? i : 2 * S - 1 - i;  // density_estimator.py:375-387 forward, :395-405 backwards
        const int upper = (c & 1) == 0;         // RealNVP(upper) first (density_estimator.py:260-270)
        const float* ps = p + (c >> 1) * fl.stage;
        int unit = 0;
        build_wide_image_io(slot, ps + (upper ? 0 : fl.p_up), wl, upper ? h : hh, upper ? hh : h, U, lane, wave, WS_WAVES, unit);
        // fold slot (half, f): the feature d = (half ? h : 0) + f when f is inside the half, else (1, 0)
        float* fold = slot + img_floats;
        for (int r = threadIdx.x; r < 32 * HT; r += WS_WAVES * 64) {
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
    };

    build(0, ws_lds);
    // the parameter-only log-dets, sum(a) - sum(log alpha) (bijectors.py:293, 417): every wave sums them for itself, in
    // flow_wide.hip's order, so that all waves (and both kernels) hold the same bits
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
    const int64_t ngroups = (ntiles + WS_WAVES * T - 1) / (WS_WAVES * T);
    // workgroup-uniform trip count: blockIdx.x, gridDim.x and ngroups are the same for all 512 threads
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const bool more = g + gridDim.x < ngroups;  // this workgroup walks another group: keep the ring going
        const int64_t tile0 = g * (WS_WAVES * T) + wave;
        // tiles tile0 + 8 t, t < nt, exist (nt is wave-uniform; a wave with nt == 0 only builds and waits)
        const int64_t left = ntiles - tile0;
        const int nt = left <= 0 ? 0 : left > (T - 1) * WS_WAVES ? T : (int)((left + WS_WAVES - 1) / WS_WAVES);
        f4 lo[T][HT], hi[T][HT];
        float ssum[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            ssum[t] = 0.f;
#pragma unroll
            for (int mm = 0; mm < HT; ++mm) lo[t][mm] = hi[t][mm] = zero;
            if (t < nt) {
                const int64_t row = (tile0 + WS_WAVES * t) * 16 + s;
                const float* zr = zb + (row < a.N ? row : a.N - 1) * D;  // a copy of the last row: computed, never stored
                if (vec_in) {
#pragma unroll
                    for (int mm = 0; mm < HT; ++mm) {
                        const int f = 16 * mm + 4 * q;
                        lo[t][mm] = f < h ? *reinterpret_cast<const f4*>(zr + f) : zero;
                        hi[t][mm] = f < h ? *reinterpret_cast<const f4*>(zr + h + f) : zero;
                    }
                } else {
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
        }
        asm volatile("" ::: "memory");  // operand reads stay inside the walk

        for (int i = 0; i < 2 * S; ++i) {
            const float* cur = ws_lds + (two ? (i & 1) : 0) * layer_floats;
            const bool upper = ((FWD ? i : 2 * S - 1 - i) & 1) == 0;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (t < nt) {
                    if (!FWD) {
                        wide_flow_fold<HT>(cur + img_floats, q, lo[t], hi[t]);
                        if (upper) wide_flow_layer<HT, UT, true, DEEP>(cur, wl, lane, lo[t], hi[t], ssum[t]);  // conditioned on the lower half
                        else wide_flow_layer<HT, UT, true, DEEP>(cur, wl, lane, hi[t], lo[t], ssum[t]);
                    } else {
                        if (upper) wide_flow_layer<HT, UT, false, DEEP>(cur, wl, lane, lo[t], hi[t], ssum[t]);
                        else wide_flow_layer<HT, UT, false, DEEP>(cur, wl, lane, hi[t], lo[t], ssum[t]);
                        wide_flow_fold<HT>(cur + img_floats, q, lo[t], hi[t]);
                    }
                }
            }
            // the next position's slot: the other one (last read at step i - 1, behind that step's barrier), or this one
            // once every wave has finished reading it
            const bool last = i == 2 * S - 1;
            if (!two) __syncthreads();
            if (!last || more) build(last ? 0 : i + 1, ws_lds + (two ? ((i + 1) & 1) : 0) * layer_floats);
            __syncthreads();
        }

#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (t < nt) {
                const int64_t row = (tile0 + WS_WAVES * t) * 16 + s;
                const bool row_ok = row < a.N;
                const float ld_tot = __builtin_fmaf(reduce_q(ssum[t]), kLn2, ldc);  // the tile code sums s log2(e)
                if (!FWD && lpo) {
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
                    float* zw = zo + row * D;
                    if (vec_out) {
#pragma unroll
                        for (int mm = 0; mm < HT; ++mm) {
                            const int f = 16 * mm + 4 * q;
                            if (f < h) {
                                *reinterpret_cast<f4*>(zw + f) = lo[t][mm];
                                *reinterpret_cast<f4*>(zw + h + f) = hi[t][mm];
                            }
                        }
                    } else {
#pragma unroll
                        for (int mm = 0; mm < HT; ++mm)
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int f = 16 * mm + 4 * q + j;
                                if (f < h) zw[f] = lo[t][mm][j];
                                if (f < hh) zw[h + f] = hi[t][mm][j];
                            }
                    }
                }
            }
        }
    }
}

static int launch_wide_stream(WideStreamArgs a, int L, bool fwd, int which, hipStream_t st) {
    const WideLayout wl = wide_flow_layout(a.D, L, a.U);
    a.slots = wide_stream_slots(a.D, L, a.U);
    const size_t smem = (size_t)wide_stream_lds_bytes(a.D, L, a.U);
    const int64_t M = a.Mz > a.Mp ? a.Mz : a.Mp;
    const int forced = g_widestream_tiles.load(std::memory_order_relaxed);
    int T = forced ? forced : wide_stream_tiles(a.D, L, a.U, M, a.N);
    const int cap = wide_stream_max_tiles(wl.HT, wl.UT, L > 3);  // a forced T the tile shape does not have: its largest
    if (T > cap) T = cap;
    // one workgroup per CU is all the LDS admits: one resident round of workgroups, each walking whole groups
    const dim3 grid = grid_xm(persistent_bx(wide_stream_groups(a.N, T), 1, 256, M), M);
    g_widestream_launches[which].fetch_add(1, std::memory_order_relaxed);
    const int rc = dispatch_bool(wl.HT > 1, [&](auto two) {
        return dispatch_range<2, 4>(wl.UT, [&](auto ut) {
            return dispatch_bool(fwd, [&](auto f) {
                return dispatch_bool(L > 3, [&](auto deep) {  // the refined activation of wide_flow_tile.h
                    return dispatch_wide_stream_tiles(T, [&](auto t) {
                        constexpr int HT = two() ? 2 : 1;
                        constexpr int TT = t() > wide_stream_max_tiles(HT, ut(), deep()) ? 1 : t();  // (never reached: clamped)
                        return launch_lds("wide_flow_stream", flow_wide_stream_kernel<HT, ut(), f(), deep(), TT>, grid,
                                          dim3(WS_WAVES * 64), smem, st, a, wl);
                    });
                });
            });
        });
    });
    if (rc != TNF_OK) return rc;
    return check_launch("wide_flow_stream");
}

// everything the two entries refuse before a launch, in the order of tnf_widestream.h (the NULL and output checks come
// first, with the callers): wideflow_checks of flow_wide.hip with this family's predicate
static int widestream_checks(const char* fn, int64_t Mz, int64_t Mp, int64_t N, int D, int S, int L, int U, int64_t pstride,
                             bool sampling) {
    const int64_t M = Mz > Mp ? Mz : Mp;
    if (Mz < 1 || Mp < 1 || (Mz != 1 && Mz != M) || (Mp != 1 && Mp != M) || (sampling && Mz != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M_z=%lld M_p=%lld N=%lld", fn, (long long)Mz, (long long)Mp, (long long)N);
    if (M > (int64_t)32768 * 65535) return fail(TNF_EINVAL, "%s: M=%lld exceeds the grid", fn, (long long)M);
    if (!wide_stream_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no streamed whole-flow wide kernel for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_wide_flow_stream_supported(int32_t D, int32_t S, int32_t L, int32_t U) {
    return wide_stream_supported(D, S, L, U) ? 1 : 0;
}

int64_t tnf_wide_flow_stream_lds_bytes(int32_t D, int32_t L, int32_t U) { return wide_stream_lds_bytes(D, L, U); }

int tnf_wide_flow_stream_tiles(int32_t D, int32_t S, int32_t L, int32_t U, int64_t M, int64_t N) {
    return wide_stream_supported(D, S, L, U) && M >= 1 && N >= 0 ? wide_stream_tiles(D, L, U, M, N) : -1;
}

int tnf_wide_flow_stream_set_tiles(int32_t T) {
    if (T != 0 && !wide_stream_tiles_shipped(T))
        return fail(TNF_EINVAL, "tnf_wide_flow_stream_set_tiles: T=%d is not 0 (the rule) or a shipped tile count", T);
    return g_widestream_tiles.exchange(T, std::memory_order_relaxed);
}

int64_t tnf_wide_flow_stream_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_WIDESTREAM_COUNTERS)
        return fail(TNF_EINVAL, "tnf_wide_flow_stream_launch_count: counter %d", which);
    return g_widestream_launches[which].load(std::memory_order_relaxed);
}

int tnf_wide_flow_stream_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                                      float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N,
                                      int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_wide_flow_stream_log_prob_f32";
    if (!z || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!log_prob && !z0 && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = widestream_checks(fn, M_z, M_p, N, D, S, L, U, pstride, false)) return rc;
    if (z0 == z) return fail(TNF_EINVAL, "%s: z0 must not alias z", fn);
    if (N == 0) return TNF_OK;
    const WideStreamArgs a{z, params, bn_mean, bn_alpha, z0, sum_log_det, log_prob, M_z, M_p, N, pstride, D, S, U, 0,
                           g_launch_gate};
    return launch_wide_stream(a, L, false, TNF_WIDESTREAM_COUNT_LOG_PROB, as_stream(stream));
}

int tnf_wide_flow_stream_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                                     float* z_out, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N, int32_t D,
                                     int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_wide_flow_stream_forward_f32";
    if (!omega || !params || !bn_mean || !bn_alpha) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!z_out && !sum_log_det) return fail(TNF_EINVAL, "%s: no output requested", fn);
    if (int rc = widestream_checks(fn, M_z, M_p, N, D, S, L, U, pstride, true)) return rc;
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    if (N == 0) return TNF_OK;
    const WideStreamArgs a{omega, params, bn_mean, bn_alpha, z_out, sum_log_det, nullptr, M_z, M_p, N, pstride, D, S, U, 0,
                           g_launch_gate};
    return launch_wide_stream(a, L, true, TNF_WIDESTREAM_COUNT_FORWARD, as_stream(stream));
}

}  // extern "C"
