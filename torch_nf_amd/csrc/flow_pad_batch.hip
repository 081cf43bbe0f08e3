// Sampling a coupling flow of any width 2 <= D <= 63 (D != 32) with fresh batch statistics in one call
// (include/tnf_padbatch.h): the flow is embedded into the one of width 2H (the layout of padtrain_map.h, moved by the
// kernels of flow_pad_train.hip) and the batch-statistics chains of coupling_mfma.hip run on the embedded problem.  The
// device work that is new:
//   padbatch_finalize_fold  flow_batch_finalize_fold_kernel for rows in the embedded layout.  BatchNorm over a padded
//                           column is not the identity -- alpha = sqrt(0 + eps) would put -log sqrt(eps) into the log-det
//                           and, at eps = 0, 0 * inf = NaN into the padding -- so a padded slot gets (mean, alpha, A, B) =
//                           (0, 1, 1, 0), adds nothing to the log-det and never forms 1 / sqrt(0 + eps).  A real slot: the
//                           statements of the existing kernel in their order (double moments, (float) casts, logf).
//   padbatch_gather_stats   (2S, 2H) mean and alpha -> the (2S, D) rows the BatchNorm layers cache
// With (0, 1) at padding the backward needs nothing new: P = sum g v and Q = sum g are 0 there (g = 0: zero weight rows,
// A = 1 on a zero gradient; v = 0), so fold_backward_ctx_kernel adds 0 to g_r and g_mu, fold_backward_fin_kernel gives
// k0 = 0 (mu = 0) and a finite k1, and g_v = g A + k0 + k1 v = 0 because v is exactly 0.  Its atomicAdd into the padded
// slots of the embedded gradient row (S_m, for an Affine layer) lands where gather_params never reads.
// Plain vector loads and stores, no atomics, no allocation, no synchronisation (capturable).
#include <atomic>

#include "launch.h"
#include "padtrain_map.h"
#include "../../include/tnf_padbatch.h"
#include "../../include/tnf_padtrain.h"

namespace tnf {

static std::atomic<long long> g_padbatch_launches[TNF_PADBATCH_COUNTERS];
static void padbatch_count(int which) { g_padbatch_launches[which].fetch_add(1, std::memory_order_relaxed); }

// One workgroup per context m; every workgroup derives the statistics itself (2H values), workgroup 0 hands them out.
// moments = [sum (2H) | sum of squares (2H) | row count]; fold (Mp, 2, 2H); ldc (Mp)
__global__ void __launch_bounds__(256)
padbatch_finalize_fold_kernel(const float* __restrict__ params, int64_t pstride, int64_t affine_off,
                              const double* __restrict__ moments, float eps, float* __restrict__ mean_out,
                              float* __restrict__ alpha_out, float* __restrict__ fold, float* __restrict__ ldc, int H, int Dr,
                              int has_affine, int first) {
    const int D = 2 * H;
    const int64_t m = blockIdx.x;
    const float* ap = params + m * pstride + affine_off;
    const double rows = moments[2 * D];
    float acc = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        if (padtrain_feature_real(d, H, Dr) < 0) {  // padding: the identity, whatever eps is
            if (m == 0) {
                mean_out[d] = 0.f;
                alpha_out[d] = 1.f;
            }
            fold[m * 2 * D + d] = 1.f;
            fold[m * 2 * D + D + d] = 0.f;
            continue;
        }
        const double mud = moments[d] / rows;
        double var_b = moments[D + d] / rows - mud * mud;
        if (var_b < 0.0) var_b = 0.0;
        const double ad = sqrt(var_b + (double)eps);
        const float mu = (float)mud, rs = (float)(1.0 / ad);
        if (m == 0) {
            mean_out[d] = mu;
            alpha_out[d] = (float)ad;
        }
        acc -= logf((float)ad);  // BatchNorm's log-det
        float A = rs, B = -mu * rs;
        if (has_affine) {
            const float av = ap[d], ea = expf(av);
            acc += av;
            A = ea * rs;
            B = ap[D + d] - mu * A;
        }
        fold[m * 2 * D + d] = A;
        fold[m * 2 * D + D + d] = B;
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) ldc[m] = (first ? 0.f : ldc[m]) + red[0];
}

// mean, alpha (rows, 2H) -> (rows, D): one thread per real value of either block
__global__ void __launch_bounds__(256)
padbatch_gather_stats_kernel(const float* __restrict__ mean, const float* __restrict__ alpha, float* __restrict__ mean_out,
                             float* __restrict__ alpha_out, int rows, int H, int Dr) {
    const int n = rows * Dr;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * n) return;
    const int which = k >= n, e = which ? k - n : k;
    const int src = (e / Dr) * 2 * H + padtrain_feature(e % Dr, H, Dr);
    (which ? alpha_out : mean_out)[e] = (which ? alpha : mean)[src];
}

// the fold of the chains of coupling_mfma.hip when they run on an embedded flow (real_D != 0 there)
int launch_pad_finalize_fold(const float* params, int64_t pstride, int64_t affine_off, const double* moments, float eps,
                             float* mean_out, float* alpha_out, float* fold, float* ldc, int64_t Mp, int W, int real_D,
                             int has_affine, int first, hipStream_t st) {
    padbatch_count(TNF_PADBATCH_COUNT_FOLD);
    hipLaunchKernelGGL(padbatch_finalize_fold_kernel, dim3((unsigned)Mp), dim3(256), 0, st, params, pstride, affine_off,
                       moments, eps, mean_out, alpha_out, fold, ldc, W / 2, real_D, has_affine, first);
    return check_launch("flow_padded_batch_fold");
}

static int launch_gather_stats(const float* mean, const float* alpha, float* mean_out, float* alpha_out, int S, int D,
                               hipStream_t st) {
    const int H = padtrain_half(D), n = 2 * 2 * S * D;
    padbatch_count(TNF_PADBATCH_COUNT_GATHER_STATS);
    hipLaunchKernelGGL(padbatch_gather_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mean, alpha,
                       mean_out, alpha_out, 2 * S, H, D);
    return check_launch("flow_padded_batch_gather_stats");
}

// workspaces.  forward: [omega' | z' | params' | mean', alpha' | the chain's own]
//              training: [omega' | g_z' | g_omega' | params' | g_params' | mean', alpha' | the pair's own]; its forward
//              uses the same block with z' in the place of g_z'
struct PadBatchWs {
    float *o, *z, *go, *p, *gp, *mean, *alpha;  // go, gp: the training block only (empty regions otherwise)
    char* inner;
    int64_t bytes;
};
static PadBatchWs padbatch_ws(int64_t M, int64_t Mp, int64_t N, int D, int S, int L, int U, bool train, void* ws) {
    const int W = 2 * padtrain_half(D);
    const int64_t rows = M * N * W, prow = Mp * flow_layout(W, S, L, U).total;
    Carver c(ws);
    PadBatchWs w;
    w.o = c.take<float>(rows, 256);
    w.z = c.take<float>(rows, 256);
    w.go = c.take<float>(train ? rows : 0, 256);
    w.p = c.take<float>(prow, 256);
    w.gp = c.take<float>(train ? prow : 0, 256);
    w.mean = c.take<float>((int64_t)2 * S * W, 256);
    w.alpha = c.take<float>((int64_t)2 * S * W, 4);
    w.inner = c.take<char>(train ? flow_forward_train_workspace(M, Mp, N > 0 ? N : 1, W, S, L)
                                 : flow_forward_batch_workspace(Mp, W, S, L), 256);
    w.bytes = c.bytes(256);
    return w;
}

// everything the three composites refuse before a launch, in the order of tnf_padbatch.h; need: the workspace size
static int padbatch_checks(const char* fn, int64_t M, int64_t Mp, int64_t N, int D, int S, int L, int U, int64_t pstride) {
    if (M < 1 || (Mp != 1 && Mp != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M=%lld M_p=%lld N=%lld", fn, (long long)M, (long long)Mp, (long long)N);
    if (!tnf_flow_padded_batch_supported(D, S, L, U))
        return fail(TNF_EUNSUPPORTED, "%s: no padded batch-statistics chain for D=%d S=%d L=%d U=%d", fn, D, S, L, U);
    const int64_t need = flow_layout(D, S, L, U).total;
    if (pstride < need)
        return fail(TNF_EINVAL, "%s: params row has %lld elements, flow needs %lld", fn, (long long)pstride, (long long)need);
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_flow_padded_batch_supported(int32_t D, int32_t S, int32_t L, int32_t U) {
    const int W = 2 * padtrain_half(D);
    return W && S >= 1 && mfma_supported(W, L, U) ? 1 : 0;
}

int64_t tnf_padbatch_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_PADBATCH_COUNTERS) return fail(TNF_EINVAL, "tnf_padbatch_launch_count: counter %d", which);
    return g_padbatch_launches[which].load(std::memory_order_relaxed);
}

int tnf_flow_padded_batch_fold_f32(const float* params, const double* moments, float* mean_out, float* alpha_out,
                                   float* fold, float* ldc, int64_t M_p, int32_t D, int64_t pstride, int64_t affine_off,
                                   int32_t has_affine, int32_t first, float eps, void* stream) {
    const char* fn = "tnf_flow_padded_batch_fold_f32";
    if (!params || !moments || !mean_out || !alpha_out || !fold || !ldc) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (M_p < 1) return fail(TNF_EINVAL, "%s: M_p=%lld", fn, (long long)M_p);
    const int W = 2 * padtrain_half(D);
    if (!W) return fail(TNF_EUNSUPPORTED, "%s: no embedded layout for D=%d", fn, D);
    if (!is_aligned(moments, 8)) return fail(TNF_EINVAL, "%s: moments must be 8-byte aligned", fn);
    if (affine_off < 0 || (has_affine && pstride < affine_off + 2 * (int64_t)W))
        return fail(TNF_EINVAL, "%s: affine_off=%lld pstride=%lld", fn, (long long)affine_off, (long long)pstride);
    return launch_pad_finalize_fold(params, pstride, affine_off, moments, eps, mean_out, alpha_out, fold, ldc, M_p, W, D,
                                    has_affine != 0, first != 0, as_stream(stream));
}

int64_t tnf_flow_padded_batch_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U) {
    const int64_t big = (int64_t)1 << 40;  // the row length is not this query's business
    if (int rc = padbatch_checks("tnf_flow_padded_batch_workspace_bytes", M, M_p, N, D, S, L, U, big)) return rc;
    return padbatch_ws(M, M_p, N, D, S, L, U, false, nullptr).bytes;
}

int64_t tnf_flow_padded_batch_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L,
                                                    int32_t U) {
    const int64_t big = (int64_t)1 << 40;
    if (int rc = padbatch_checks("tnf_flow_padded_batch_train_workspace_bytes", M, M_p, N, D, S, L, U, big)) return rc;
    return padbatch_ws(M, M_p, N, D, S, L, U, true, nullptr).bytes;
}

int tnf_flow_padded_forward_batch_f32(const float* omega, const float* params, float* z_out, float* sum_log_det,
                                      float* bn_mean_out, float* bn_alpha_out, int64_t M, int64_t M_p, int64_t N, int32_t D,
                                      int32_t S, int32_t L, int32_t U, int64_t pstride, float eps, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_flow_padded_forward_batch_f32";
    if (int rc = padbatch_checks(fn, M, M_p, N, D, S, L, U, pstride)) return rc;
    if (N == 0) return TNF_OK;
    if (M * N < 2) return fail(TNF_EINVAL, "%s: batch statistics need more than one row", fn);
    if (!omega || !params || !z_out || !sum_log_det || !bn_mean_out || !bn_alpha_out)
        return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    const PadBatchWs w = padbatch_ws(M, M_p, N, D, S, L, U, false, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes, 256)) return rc;
    hipStream_t st = as_stream(stream);
    const int W = 2 * padtrain_half(D);
    const int64_t pe_stride = flow_layout(W, S, L, U).total;
    float *oe = w.o, *ze = w.z, *pe = w.p, *mean_e = w.mean, *alpha_e = w.alpha;
    void* inner = w.inner;
    padbatch_count(TNF_PADBATCH_COUNT_FORWARD);
    int rc = launch_embed_rows(omega, oe, M * N, D, st);
    if (rc) return rc;
    rc = launch_embed_params(params, nullptr, nullptr, pe, nullptr, nullptr, M_p, D, S, L, U, pstride, st);
    if (rc) return rc;
    rc = flow_forward_batch_begin(pe, M_p, W, S, L, U, pe_stride, inner, st);
    if (rc) return rc;
    for (int c = 0; c < 2 * S; ++c) {
        rc = flow_forward_batch_layer(c, c == 0 ? oe : ze, pe, ze, sum_log_det, nullptr, M, M_p, N, W, S, L, U, pe_stride,
                                      inner, st);
        if (rc) return rc;
        rc = flow_forward_batch_fold(c, pe, nullptr, mean_e, alpha_e, M_p, W, S, L, U, pe_stride, eps, inner, st, D);
        if (rc) return rc;
    }
    rc = flow_forward_batch_end(ze, sum_log_det, M, M_p, N, W, S, L, inner, st);
    if (rc) return rc;
    rc = launch_gather_rows(ze, z_out, M * N, D, st);
    if (rc) return rc;
    return launch_gather_stats(mean_e, alpha_e, bn_mean_out, bn_alpha_out, S, D, st);
}

int tnf_flow_padded_forward_train_fwd_f32(const float* omega, const float* params, float* z_out, float* sum_log_det,
                                          float* states, float* folds, float* bn_mean_out, float* bn_alpha_out, int64_t M,
                                          int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride,
                                          float eps, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_flow_padded_forward_train_fwd_f32";
    if (int rc = padbatch_checks(fn, M, M_p, N, D, S, L, U, pstride)) return rc;
    if (N == 0) return TNF_OK;
    if (M * N < 2) return fail(TNF_EINVAL, "%s: batch statistics need more than one row", fn);
    if (!omega || !params || !z_out || !sum_log_det || !states || !folds || !bn_mean_out || !bn_alpha_out)
        return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!is_aligned(states, 16)) return fail(TNF_EINVAL, "%s: states must be 16-byte aligned", fn);
    const PadBatchWs w = padbatch_ws(M, M_p, N, D, S, L, U, true, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes, 256)) return rc;
    hipStream_t st = as_stream(stream);
    const int W = 2 * padtrain_half(D);
    const int64_t pe_stride = flow_layout(W, S, L, U).total;
    float *oe = w.o, *ze = w.z, *pe = w.p, *mean_e = w.mean, *alpha_e = w.alpha;
    padbatch_count(TNF_PADBATCH_COUNT_TRAIN_FWD);
    int rc = launch_embed_rows(omega, oe, M * N, D, st);
    if (rc) return rc;
    rc = launch_embed_params(params, nullptr, nullptr, pe, nullptr, nullptr, M_p, D, S, L, U, pstride, st);
    if (rc) return rc;
    rc = launch_flow_forward_train_fwd(oe, pe, ze, sum_log_det, states, folds, mean_e, alpha_e, M, M_p, N, W, S, L, U,
                                       pe_stride, eps, w.inner, st, D);
    if (rc) return rc;
    rc = launch_gather_rows(ze, z_out, M * N, D, st);
    if (rc) return rc;
    return launch_gather_stats(mean_e, alpha_e, bn_mean_out, bn_alpha_out, S, D, st);
}

int tnf_flow_padded_forward_train_bwd_f32(const float* omega, const float* params, const float* states, const float* folds,
                                          const float* bn_mean, const float* bn_alpha, const float* g_z,
                                          const float* g_sum_log_det, float* g_omega, float* g_params, int64_t M, int64_t M_p,
                                          int64_t N, int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride,
                                          int64_t gpstride, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_flow_padded_forward_train_bwd_f32";
    if (int rc = padbatch_checks(fn, M, M_p, N, D, S, L, U, pstride)) return rc;
    if (gpstride < flow_layout(D, S, L, U).total) return fail(TNF_EINVAL, "%s: g_params row too short", fn);
    if (N == 0) return TNF_OK;
    if (M * N < 2) return fail(TNF_EINVAL, "%s: batch statistics need more than one row", fn);
    if (!omega || !params || !states || !folds || !bn_mean || !bn_alpha || !g_z || !g_sum_log_det || !g_params)
        return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!is_aligned(states, 16)) return fail(TNF_EINVAL, "%s: states must be 16-byte aligned", fn);
    const PadBatchWs w = padbatch_ws(M, M_p, N, D, S, L, U, true, workspace);
    if (int rc = check_workspace(fn, workspace, workspace_bytes, w.bytes, 256)) return rc;
    hipStream_t st = as_stream(stream);
    const int W = 2 * padtrain_half(D);
    const int64_t pe_stride = flow_layout(W, S, L, U).total;
    float *oe = w.o, *gze = w.z, *goe = g_omega ? w.go : nullptr, *pe = w.p, *gpe = w.gp, *mean_e = w.mean, *alpha_e = w.alpha;
    padbatch_count(TNF_PADBATCH_COUNT_TRAIN_BWD);
    int rc = launch_embed_rows(omega, oe, M * N, D, st);
    if (rc) return rc;
    rc = launch_embed_rows(g_z, gze, M * N, D, st);  // zeros at padding: P = Q = 0 there
    if (rc) return rc;
    rc = launch_embed_params(params, bn_mean, bn_alpha, pe, mean_e, alpha_e, M_p, D, S, L, U, pstride, st);
    if (rc) return rc;
    // the backward's callers hand it a zeroed gradient row (ops.py): the same here, so that the embedded call is that call
    if (hipMemsetAsync(gpe, 0, (size_t)(M_p * pe_stride) * sizeof(float), st) != hipSuccess)
        return fail(TNF_ELAUNCH, "%s: memset failed", fn);
    rc = launch_flow_forward_train_bwd(oe, pe, states, folds, mean_e, alpha_e, gze, g_sum_log_det, goe, gpe, M, M_p, N, W, S,
                                       L, U, pe_stride, pe_stride, w.inner, st);
    if (rc) return rc;
    rc = launch_gather_params(gpe, g_params, M_p, D, S, L, U, gpstride, st);
    if (rc) return rc;
    return g_omega ? launch_gather_rows(goe, g_omega, M * N, D, st) : TNF_OK;
}

}  // extern "C"
