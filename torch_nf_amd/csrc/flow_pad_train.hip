// Training a coupling flow of any width 2 <= D <= 63 (D != 32) through the reversible backward of flow_bwd_f16.hip
// (include/tnf_padtrain.h): the flow is embedded into the one of width 2H (H = 16 or 32) with zeros in the extra slots,
// the existing kernel runs on the embedded problem, and the gradients are read back from the real slots.  The only device
// work here is moving rows and parameter rows into and out of the embedded layout (padtrain_map.h):
//   embed_rows     one thread per 16 bytes of the embedded side: coalesced 4-byte loads of the real row, one 16-byte
//                  store, zeros included (no memset); quads that are all padding load nothing
//   gather_rows    the inverse: 16-byte loads of the quads that hold a real feature, 4-byte stores
//   embed_params   one thread per REAL parameter: it stores its value at the image of its index and the zeros of the gap
//                  up to the next image (the map is strictly increasing, so the gaps are exactly the padding: at most
//                  15 * 16 floats after a first layer's last row); the same launch embeds the (2S, D) statistics
//   gather_params  one thread per real parameter, reading only its image: the padded slots of a gradient row hold sums
//                  that belong to no parameter
// Memory-bound copies: 4 * R * (D + 2H) bytes per row kernel.  Grid-stride loops, 64-bit indices, plain vector loads
// and stores; no atomics, no allocation, no synchronisation (capturable).
#include <atomic>

#include "launch.h"
#include "padtrain_map.h"
#include "../../include/tnf_padtrain.h"

namespace tnf {

static std::atomic<long long> g_padtrain_launches[TNF_PADTRAIN_COUNTERS];
static void padtrain_count(int which) { g_padtrain_launches[which].fetch_add(1, std::memory_order_relaxed); }

typedef float f4 __attribute__((ext_vector_type(4)));

template <int H>
__global__ void __launch_bounds__(256) padtrain_embed_rows_kernel(const float* __restrict__ rows, float* __restrict__ out,
                                                                  int64_t R, int D) {
    constexpr int Q = 2 * H / 4;  // 16-byte quads per embedded row
    const int64_t total = R * Q, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / Q;
        const int pf = 4 * (int)(i % Q);
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (padtrain_feature_real(pf, H, D) >= 0) {  // 4 | H: a quad lies in one half, real features come first in it
            const float* src = rows + r * D;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = padtrain_feature_real(pf + j, H, D);
                if (d >= 0) v[j] = src[d];
            }
        }
        *reinterpret_cast<f4*>(out + 4 * i) = v;
    }
}

template <int H>
__global__ void __launch_bounds__(256) padtrain_gather_rows_kernel(const float* __restrict__ rows, float* __restrict__ out,
                                                                   int64_t R, int D) {
    constexpr int Q = 2 * H / 4;
    const int64_t total = R * Q, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const int64_t r = i / Q;
        const int pf = 4 * (int)(i % Q);
        if (padtrain_feature_real(pf, H, D) < 0) continue;  // all padding: not read
        const f4 v = *reinterpret_cast<const f4*>(rows + 4 * i);
        float* dst = out + r * D;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = padtrain_feature_real(pf + j, H, D);
            if (d >= 0) dst[d] = v[j];
        }
    }
}

struct PadParamArgs {
    const float* params;  // (Mp, pstride)
    const float* bn_mean;  // (2S, D)
    const float* bn_alpha;
    float* params_out;  // (Mp, fe.total)
    float* bn_mean_out;  // (2S, 2H)
    float* bn_alpha_out;
    int64_t pstride;
    int D, H, S, L, U;
    FlowLayout fr, fe;
};

// grid.x covers the real row and then the two embedded statistics blocks (written by context 0's workgroups)
__global__ void __launch_bounds__(256) padtrain_embed_params_kernel(PadParamArgs a) {
    const int64_t m = grid_m();
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < a.fr.total) {
        float* dst = a.params_out + m * a.fe.total;
        const int64_t e = padtrain_embed_index(k, a.D, a.H, a.L, a.U, a.fr, a.fe);
        const int64_t next = k + 1 < a.fr.total ? padtrain_embed_index(k + 1, a.D, a.H, a.L, a.U, a.fr, a.fe) : a.fe.total;
        dst[e] = a.params[m * a.pstride + k];
        for (int64_t p = e + 1; p < next; ++p) dst[p] = 0.f;
        return;
    }
    const int W = 2 * a.H;
    const int64_t nstat = (int64_t)2 * a.S * W;
    const int64_t t = k - a.fr.total;
    if (m != 0 || t >= 2 * nstat) return;
    const int which = t >= nstat;  // 0: mean (0 at padding), 1: alpha (1 at padding)
    const int64_t e = which ? t - nstat : t;
    const int d = padtrain_feature_real((int)(e % W), a.H, a.D);
    const float* src = which ? a.bn_alpha : a.bn_mean;
    (which ? a.bn_alpha_out : a.bn_mean_out)[e] = d >= 0 ? src[(e / W) * a.D + d] : (which ? 1.f : 0.f);
}

__global__ void __launch_bounds__(256) padtrain_gather_params_kernel(const float* __restrict__ g, float* __restrict__ g_out,
                                                                     int64_t gpstride, int D, int H, int L, int U,
                                                                     FlowLayout fr, FlowLayout fe) {
    const int64_t m = grid_m();
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < fr.total) g_out[m * gpstride + k] = g[m * fe.total + padtrain_embed_index(k, D, H, L, U, fr, fe)];
}

static unsigned rows_grid(int64_t R, int H) {
    const int64_t blocks = (R * (2 * H / 4) + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks));  // grid-stride beyond 32 workgroups per CU
}

// the launchers: arguments checked by the entries (tnf_common.h: flow_pad_batch.hip composes them too)
int launch_embed_rows(const float* rows, float* out, int64_t R, int D, hipStream_t st) {
    const int H = padtrain_half(D);
    padtrain_count(TNF_PADTRAIN_COUNT_EMBED_ROWS);
    if (H == 16) hipLaunchKernelGGL(padtrain_embed_rows_kernel<16>, dim3(rows_grid(R, H)), dim3(256), 0, st, rows, out, R, D);
    else hipLaunchKernelGGL(padtrain_embed_rows_kernel<32>, dim3(rows_grid(R, H)), dim3(256), 0, st, rows, out, R, D);
    return check_launch("flow_padded_embed_rows");
}

int launch_gather_rows(const float* rows, float* out, int64_t R, int D, hipStream_t st) {
    const int H = padtrain_half(D);
    padtrain_count(TNF_PADTRAIN_COUNT_GATHER_ROWS);
    if (H == 16) hipLaunchKernelGGL(padtrain_gather_rows_kernel<16>, dim3(rows_grid(R, H)), dim3(256), 0, st, rows, out, R, D);
    else hipLaunchKernelGGL(padtrain_gather_rows_kernel<32>, dim3(rows_grid(R, H)), dim3(256), 0, st, rows, out, R, D);
    return check_launch("flow_padded_gather_rows");
}

int launch_embed_params(const float* params, const float* bn_mean, const float* bn_alpha, float* params_out,
                        float* bn_mean_out, float* bn_alpha_out, int64_t Mp, int D, int S, int L, int U, int64_t pstride,
                        hipStream_t st) {
    const int H = padtrain_half(D);
    const int Ss = bn_mean ? S : 0;  // bn_mean == NULL: the parameter rows alone (no statistics block, none is read)
    PadParamArgs a{params, bn_mean, bn_alpha, params_out, bn_mean_out, bn_alpha_out, pstride, D, H, Ss, L, U,
                   flow_layout(D, S, L, U), flow_layout(2 * H, S, L, U)};
    const int64_t threads = a.fr.total + (int64_t)2 * 2 * Ss * 2 * H;
    padtrain_count(TNF_PADTRAIN_COUNT_EMBED_PARAMS);
    hipLaunchKernelGGL(padtrain_embed_params_kernel, grid_xm((threads + 255) / 256, Mp), dim3(256), 0, st, a);
    return check_launch("flow_padded_embed_params");
}

int launch_gather_params(const float* g, float* g_out, int64_t Mp, int D, int S, int L, int U, int64_t gpstride,
                         hipStream_t st) {
    const int H = padtrain_half(D);
    const FlowLayout fr = flow_layout(D, S, L, U), fe = flow_layout(2 * H, S, L, U);
    padtrain_count(TNF_PADTRAIN_COUNT_GATHER_PARAMS);
    hipLaunchKernelGGL(padtrain_gather_params_kernel, grid_xm((fr.total + 255) / 256, Mp), dim3(256), 0, st, g, g_out,
                       gpstride, D, H, L, U, fr, fe);
    return check_launch("flow_padded_gather_params");
}

// workspace of the composite: [z0' | g_z' | params' | g_params' | mean', alpha' | the backward's own]
struct PadTrainWs {
    float *z0, *gz, *p, *gp, *mean, *alpha;
    char* rev;
    int64_t bytes;
};
static PadTrainWs padtrain_ws(int64_t M, int64_t Mp, int64_t N, int D, int S, int L, int U, void* ws) {
    const int W = 2 * padtrain_half(D);
    const int64_t rows = M * N * W, prow = Mp * flow_layout(W, S, L, U).total;
    Carver c(ws);
    PadTrainWs w;
    w.z0 = c.take<float>(rows, 256);
    w.gz = c.take<float>(rows, 256);
    w.p = c.take<float>(prow, 256);
    w.gp = c.take<float>(prow, 256);
    w.mean = c.take<float>((int64_t)2 * S * W, 256);
    w.alpha = c.take<float>((int64_t)2 * S * W, 4);
    w.rev = c.take<char>(flow_train_rev_workspace(M, Mp, N > 0 ? N : 1, W, S, L, U), 256);
    w.bytes = c.bytes();
    return w;
}

static int check_rows(const char* fn, const float* rows, const float* out, const float* embedded, int64_t R, int D) {
    if (!rows || !out) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (R < 0) return fail(TNF_EINVAL, "%s: R=%lld", fn, (long long)R);
    if (!padtrain_half(D)) return fail(TNF_EUNSUPPORTED, "%s: no embedded layout for D=%d", fn, D);
    if (!is_aligned(embedded, 16)) return fail(TNF_EINVAL, "%s: the embedded rows must be 16-byte aligned", fn);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_flow_padded_width(int32_t D) { return 2 * padtrain_half(D); }

int tnf_flow_padded_train_supported(int32_t D, int32_t S, int32_t L, int32_t U) {
    const int W = 2 * padtrain_half(D);
    return W && tnf_flow_padded_supported(D, S, L, U) && tnf_flow_train_rev_supported(W, S, L, U) ? 1 : 0;
}

int64_t tnf_flow_padded_embed_index(int32_t D, int32_t S, int32_t L, int32_t U, int64_t k) {
    const int H = padtrain_half(D);
    if (!H || S < 1 || L < 1 || U < 1) return -1;
    const FlowLayout fr = flow_layout(D, S, L, U);
    if (k < 0 || k >= fr.total) return -1;
    return padtrain_embed_index(k, D, H, L, U, fr, flow_layout(2 * H, S, L, U));
}

int64_t tnf_padtrain_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_PADTRAIN_COUNTERS) return fail(TNF_EINVAL, "tnf_padtrain_launch_count: counter %d", which);
    return g_padtrain_launches[which].load(std::memory_order_relaxed);
}

int tnf_flow_padded_embed_rows_f32(const float* rows, float* out, int64_t R, int32_t D, void* stream) {
    if (int rc = check_rows("tnf_flow_padded_embed_rows_f32", rows, out, out, R, D)) return rc;
    if (R == 0) return TNF_OK;
    return launch_embed_rows(rows, out, R, D, as_stream(stream));
}

int tnf_flow_padded_gather_rows_f32(const float* rows, float* out, int64_t R, int32_t D, void* stream) {
    if (int rc = check_rows("tnf_flow_padded_gather_rows_f32", rows, out, rows, R, D)) return rc;
    if (R == 0) return TNF_OK;
    return launch_gather_rows(rows, out, R, D, as_stream(stream));
}

int tnf_flow_padded_embed_params_f32(const float* params, const float* bn_mean, const float* bn_alpha, float* params_out,
                                     float* bn_mean_out, float* bn_alpha_out, int64_t M_p, int32_t D, int32_t S, int32_t L,
                                     int32_t U, int64_t pstride, void* stream) {
    const char* fn = "tnf_flow_padded_embed_params_f32";
    if (!params || !bn_mean || !bn_alpha || !params_out || !bn_mean_out || !bn_alpha_out)
        return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (M_p < 0) return fail(TNF_EINVAL, "%s: M_p=%lld", fn, (long long)M_p);
    if (!tnf_flow_padded_train_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no padded training for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    if (pstride < flow_layout(D, S, L, U).total)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride,
                    (long long)flow_layout(D, S, L, U).total);
    if (M_p == 0) return TNF_OK;
    return launch_embed_params(params, bn_mean, bn_alpha, params_out, bn_mean_out, bn_alpha_out, M_p, D, S, L, U, pstride,
                               as_stream(stream));
}

int tnf_flow_padded_gather_params_f32(const float* g, float* g_out, int64_t M_p, int32_t D, int32_t S, int32_t L, int32_t U,
                                      int64_t gpstride, void* stream) {
    const char* fn = "tnf_flow_padded_gather_params_f32";
    if (!g || !g_out) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (M_p < 0) return fail(TNF_EINVAL, "%s: M_p=%lld", fn, (long long)M_p);
    if (!tnf_flow_padded_train_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no padded training for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    if (gpstride < flow_layout(D, S, L, U).total)
        return fail(TNF_EINVAL, "%s: g_out row has %lld elements, flow needs %lld", fn, (long long)gpstride,
                    (long long)flow_layout(D, S, L, U).total);
    if (M_p == 0) return TNF_OK;
    return launch_gather_params(g, g_out, M_p, D, S, L, U, gpstride, as_stream(stream));
}

static int padtrain_shape(const char* fn, int64_t M, int64_t M_p, int64_t N, int D, int S, int L, int U) {
    if (M < 1 || (M_p != 1 && M_p != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M=%lld M_p=%lld N=%lld", fn, (long long)M, (long long)M_p, (long long)N);
    if (!tnf_flow_padded_train_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no padded training for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    return TNF_OK;
}

int64_t tnf_flow_padded_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U) {
    if (int rc = padtrain_shape("tnf_flow_padded_train_workspace_bytes", M, M_p, N, D, S, L, U)) return rc;
    return padtrain_ws(M, M_p, N, D, S, L, U, nullptr).bytes;
}

int tnf_flow_padded_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                     const float* g_log_prob, float* g_z, float* g_params, int64_t M, int64_t M_p, int64_t N,
                                     int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                                     void* workspace, int64_t workspace_bytes, int32_t* overflow, void* stream) {
    const char* fn = "tnf_flow_padded_log_prob_bwd_f32";
    if (int rc = padtrain_shape(fn, M, M_p, N, D, S, L, U)) return rc;
    const FlowLayout fr = flow_layout(D, S, L, U);
    if (pstride < fr.total)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride,
                    (long long)fr.total);
    if (gpstride < fr.total) return fail(TNF_EINVAL, "%s: g_params row too short", fn);
    if (N == 0) return TNF_OK;
    if (!z0 || !params || !bn_mean || !bn_alpha || !g_log_prob || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    const PadTrainWs w = padtrain_ws(M, M_p, N, D, S, L, U, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes)) return rc;
    if (!is_aligned(workspace, 16)) return fail(TNF_EINVAL, "%s: the workspace must be 16-byte aligned", fn);
    hipStream_t st = as_stream(stream);
    const int W = 2 * padtrain_half(D);
    const FlowLayout fe = flow_layout(W, S, L, U);
    float *z0e = w.z0, *gze = g_z ? w.gz : nullptr, *pe = w.p, *gpe = w.gp, *mean_e = w.mean, *alpha_e = w.alpha;
    padtrain_count(TNF_PADTRAIN_COUNT_BWD);
    int rc = launch_embed_rows(z0, z0e, M * N, D, st);
    if (rc) return rc;
    rc = launch_embed_params(params, bn_mean, bn_alpha, pe, mean_e, alpha_e, M_p, D, S, L, U, pstride, st);
    if (rc) return rc;
    // the backward's callers hand it a zeroed gradient row (ops.py): the same here, so that the embedded call is that call
    if (hipMemsetAsync(gpe, 0, (size_t)(M_p * fe.total) * sizeof(float), st) != hipSuccess)
        return fail(TNF_ELAUNCH, "%s: memset failed", fn);
    rc = launch_flow_bwd_rev(z0e, pe, mean_e, alpha_e, g_log_prob, gze, gpe, M, M_p, N, W, S, L, U, fe.total, fe.total,
                             w.rev, overflow, st);
    if (rc) return rc;
    rc = launch_gather_params(gpe, g_params, M_p, D, S, L, U, gpstride, st);
    if (rc) return rc;
    return g_z ? launch_gather_rows(gze, g_z, M * N, D, st) : TNF_OK;
}

}  // extern "C"
