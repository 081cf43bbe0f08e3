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
// The kernel's text is maf_sample_bwd_body.h, included once per mode: maf_sample_bwd_kernel (the two modes above) and
// maf_sample_bwd_batch_kernel (tnf_arbatch.h: the stack with fresh batch statistics, launch_maf_sample_bwd_batch).
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

#define MAF_SAMPLE_BWD_KERNEL maf_sample_bwd_kernel
#define MAF_SAMPLE_BWD_BATCH false
#include "maf_sample_bwd_body.h"
#undef MAF_SAMPLE_BWD_KERNEL
#undef MAF_SAMPLE_BWD_BATCH
#define MAF_SAMPLE_BWD_KERNEL maf_sample_bwd_batch_kernel
#define MAF_SAMPLE_BWD_BATCH true
#include "maf_sample_bwd_body.h"
#undef MAF_SAMPLE_BWD_KERNEL
#undef MAF_SAMPLE_BWD_BATCH

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

static int launch_maf_sample_bwd(MafSampleBwdArgs& a, hipStream_t st, bool batch = false) {
    const MafBLayout wl = maf_blayout(a.D, a.L, a.U);
    a.nacc = maf_bwd_nacc(a.D, a.L, a.U);
    const size_t smem = maf_bwd_smem(wl, a.nacc);
    const dim3 grid = maf_bwd_grid(a.M, a.Mp, a.N);
    auto go = [&](auto dt) {  // D <= 32: one or two feature tiles
        return dispatch_1to4(wl.UT, [&](auto ut) {
            return dispatch_bool(maf_sample_bwd_vec(a), [&](auto vec) {
                if (batch)
                    return launch_lds("maf_sample_bwd_batch", maf_sample_bwd_batch_kernel<dt(), ut(), vec()>, grid, dim3(256),
                                      smem, st, a, wl);
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

// the walk of tnf_ar_flow_batch_bwd_f32 (ar_flow_batch.hip): rows z, cotangents g_z / g_sld, coef (Mp, 5, D)
int launch_maf_sample_bwd_batch(const float* z, const float* params, const float* masks, const float* g_z,
                                const float* g_sld, const float* coef, float* g_params, int64_t M, int64_t Mp, int64_t N,
                                int D, int L, int U, int64_t pstride, int64_t gpstride, hipStream_t st) {
    MafSampleBwdArgs a = {};
    a.x = z; a.params = params; a.masks = masks; a.g_x = g_z; a.g_ld = g_sld; a.g_params = g_params;
    a.M = M; a.Mp = Mp; a.N = N; a.pstride = pstride; a.gpstride = gpstride; a.D = D; a.L = L; a.U = U;
    a.fold = coef;
    return launch_maf_sample_bwd(a, st, true);
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
