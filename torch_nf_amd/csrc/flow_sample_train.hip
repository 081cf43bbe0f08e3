// The C entries of include/tnf_sampletrain.h: the backward of frozen-statistics sampling in one walk kernel
// (flow_sample_bwd_kernel, flow_bwd_f16.hip).  At D = 32 / 64 the call is that launcher; at every other width
// 2 <= D <= 63 it is composed here from the embed / gather kernels of flow_pad_train.hip around the walk at the embedded
// width 2H, as tnf_flow_padded_log_prob_bwd_f32 composes the inverse direction.  No kernel of its own.
#include <atomic>

#include "launch.h"
#include "padtrain_map.h"
#include "../../include/tnf_sampletrain.h"

namespace tnf {

static std::atomic<long long> g_sampletrain_launches;

// workspace, described once: [z' | g_z' | omega' | params' | g_params' | mean', alpha' | the walk's own]; at D = 32 / 64
// nothing is embedded and only the last region has a size
struct SampleTrainWs {
    float *z, *gz, *om, *p, *gp, *mean, *alpha;
    char* rev;
    int64_t bytes;
};
static SampleTrainWs sampletrain_ws(int64_t M, int64_t Mp, int64_t N, int D, int S, int L, int U, void* ws) {
    const int H = padtrain_half(D);
    const int W = H ? 2 * H : D;
    const int64_t rows = H ? M * N * W : 0, prow = H ? Mp * flow_layout(W, S, L, U).total : 0;
    const int64_t stat = H ? (int64_t)2 * S * W : 0;
    Carver c(ws);
    SampleTrainWs w;
    w.z = c.take<float>(rows, 256);
    w.gz = c.take<float>(rows, 256);
    w.om = c.take<float>(rows, 256);
    w.p = c.take<float>(prow, 256);
    w.gp = c.take<float>(prow, 256);
    w.mean = c.take<float>(stat, 256);
    w.alpha = c.take<float>(stat, 4);
    w.rev = c.take<char>(flow_train_rev_workspace(M, Mp, N > 0 ? N : 1, W, S, L, U), 256);
    w.bytes = c.bytes();
    return w;
}

static int sampletrain_shape(const char* fn, int64_t M, int64_t M_p, int64_t N, int D, int S, int L, int U) {
    if (M < 1 || (M_p != 1 && M_p != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M=%lld M_p=%lld N=%lld", fn, (long long)M, (long long)M_p, (long long)N);
    if (!tnf_flow_sample_train_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no sampling backward for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_flow_sample_train_supported(int32_t D, int32_t S, int32_t L, int32_t U) {
    return (tnf_flow_train_rev_supported(D, S, L, U) || tnf_flow_padded_train_supported(D, S, L, U)) ? 1 : 0;
}

int64_t tnf_flow_sample_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U) {
    if (int rc = sampletrain_shape("tnf_flow_sample_train_workspace_bytes", M, M_p, N, D, S, L, U)) return rc;
    return sampletrain_ws(M, M_p, N, D, S, L, U, nullptr).bytes;
}

int64_t tnf_sampletrain_launch_count(void) { return g_sampletrain_launches.load(std::memory_order_relaxed); }

int tnf_flow_sample_bwd_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                            const float* g_z, const float* g_sld, float* g_params, float* omega_out, int64_t M, int64_t M_p,
                            int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                            void* workspace, int64_t workspace_bytes, int32_t* overflow, void* stream) {
    const char* fn = "tnf_flow_sample_bwd_f32";
    if (!z || !params || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: g_z and g_sld are both NULL", fn);
    if (int rc = sampletrain_shape(fn, M, M_p, N, D, S, L, U)) return rc;
    const FlowLayout fr = flow_layout(D, S, L, U);
    if (pstride < fr.total)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride,
                    (long long)fr.total);
    if (gpstride < fr.total) return fail(TNF_EINVAL, "%s: g_params row too short", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (omega_out == z) return fail(TNF_EINVAL, "%s: omega_out must not alias z", fn);
    const SampleTrainWs w = sampletrain_ws(M, M_p, N, D, S, L, U, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes)) return rc;
    if (!is_aligned(workspace, 16)) return fail(TNF_EINVAL, "%s: the workspace must be 16-byte aligned", fn);
    if (N == 0) return TNF_OK;
    hipStream_t st = as_stream(stream);
    const int H = padtrain_half(D);
    if (!H) {  // D = 32 / 64: the walk on the caller's rows
        if (!is_aligned(z, 16) || (g_z && !is_aligned(g_z, 16)) || (omega_out && !is_aligned(omega_out, 16)))
            return fail(TNF_EINVAL, "%s: z / g_z / omega_out must be 16-byte aligned", fn);
        const int rc = launch_flow_sample_bwd(z, params, bn_mean, bn_alpha, g_z, g_sld, g_params, omega_out, M, M_p, N, D, S,
                                              L, U, pstride, gpstride, w.rev, overflow, st);
        if (rc == TNF_OK) g_sampletrain_launches.fetch_add(1, std::memory_order_relaxed);
        return rc;
    }
    const int W = 2 * H;
    const FlowLayout fe = flow_layout(W, S, L, U);
    int rc = launch_embed_rows(z, w.z, M * N, D, st);
    if (rc) return rc;
    if (g_z) {
        rc = launch_embed_rows(g_z, w.gz, M * N, D, st);
        if (rc) return rc;
    }
    rc = launch_embed_params(params, bn_mean, bn_alpha, w.p, w.mean, w.alpha, M_p, D, S, L, U, pstride, st);
    if (rc) return rc;
    // the walk accumulates into its gradient rows: zeroed here, so that the embedded call is the call at width 2H
    if (hipMemsetAsync(w.gp, 0, (size_t)(M_p * fe.total) * sizeof(float), st) != hipSuccess)
        return fail(TNF_ELAUNCH, "%s: memset failed", fn);
    rc = launch_flow_sample_bwd(w.z, w.p, w.mean, w.alpha, g_z ? w.gz : nullptr, g_sld, w.gp, omega_out ? w.om : nullptr, M,
                                M_p, N, W, S, L, U, fe.total, fe.total, w.rev, overflow, st);
    if (rc) return rc;
    g_sampletrain_launches.fetch_add(1, std::memory_order_relaxed);
    rc = launch_gather_params(w.gp, g_params, M_p, D, S, L, U, gpstride, st);
    if (rc) return rc;
    return omega_out ? launch_gather_rows(w.om, omega_out, M * N, D, st) : TNF_OK;
}

}  // extern "C"
