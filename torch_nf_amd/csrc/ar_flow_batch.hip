// NormFlow('AR') = [MAF, BatchNorm, Affine] sampled with FRESH batch statistics, one C call each way
// (include/tnf_arbatch.h).  Forward: the matrix-pipe MAF kernel (maf_mfma.hip, unchanged, no fold behind it), the double
// moments of its output (generic_kernels.hip), ar_batch_finalize_fold_kernel, ar_batch_apply_kernel.  Backward:
// ar_batch_bwd_sums_kernel, ar_batch_bwd_combine_kernel, ar_batch_bwd_finalize_kernel and the batch mode of the sampling
// backward walk (maf_sample_bwd.hip).  With y = (z - b) e^-a the BatchNorm output and n = M N:
//   g_y = g_z e^a,  P = sum g_y,  Q = sum g_y y = sum g_z (z - b),  G = sum g_sld  (BatchNorm's log-det -sum log alpha is
//   0-dim: every row's cotangent reaches it, and d(-log alpha)/dx_i = -y_i / (n alpha))
//   g_x = (g_y - P / n - y (Q + G) / n) / alpha = g_z C0 + C1 + z C2
// The sums are double and free of atomics: a workgroup adds a fixed slice of rows in row order, the partials are added in
// workgroup order.  Every per-context quantity the global sums need (GZ, GB, GS) is also what the Affine gradient needs,
// so one pass over z and g_z serves both.
#include <atomic>

#include "launch.h"
#include "../../include/tnf_arbatch.h"

namespace tnf {

static std::atomic<long long> g_arbatch_counts[TNF_ARBATCH_COUNTERS];
static void arbatch_count(int which, long long by) { g_arbatch_counts[which].fetch_add(by, std::memory_order_relaxed); }

// ---- forward -------------------------------------------------------------------------------------------------------------
// One workgroup per parameter row; every workgroup derives the statistics itself (D values), workgroup 0 hands them out.
// The statements of flow_batch_finalize_fold_kernel (coupling_mfma.hip) with the Affine layer behind the BatchNorm; the row
// count is an argument (the caller's M N, what launch_bn_moments would have written behind the sums).
__global__ void __launch_bounds__(256)
ar_batch_finalize_fold_kernel(const float* __restrict__ params, int64_t pstride, int64_t p_maf,
                              const double* __restrict__ moments, double rows, float eps, float* __restrict__ mean_out,
                              float* __restrict__ alpha_out, float* __restrict__ fold, float* __restrict__ ldc, int D) {
    const int64_t m = blockIdx.x;
    const float* ap = params + m * pstride + p_maf;
    float acc = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
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
        const float av = ap[d], ea = expf(av);
        acc += av;
        const float A = ea * rs;
        fold[m * 2 * D + d] = A;
        fold[m * 2 * D + D + d] = ap[D + d] - mu * A;
    }
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) ldc[m] = red[0];
}

// in place z <- z A[m] + B[m], sum_log_det[m][n] += ldc[m]; VEC: four features per access (D % 4 == 0, z 16-byte aligned)
template <bool VEC>
__global__ void __launch_bounds__(256)
ar_batch_apply_kernel(float* __restrict__ z, float* __restrict__ sld, const float* __restrict__ fold,
                      const float* __restrict__ ldc, int64_t M, int64_t Mp, int64_t N, int D) {
    __shared__ __attribute__((aligned(16))) float ab[2 * 64];  // D <= 64
    const int64_t m = grid_m();
    if (m >= M) return;
    const int64_t mp = Mp == 1 ? 0 : m;
    for (int i = threadIdx.x; i < 2 * D; i += 256) ab[i] = fold[mp * 2 * D + i];
    __syncthreads();
    float* zr = z + m * N * D;
    const int64_t start = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t total = N * D / 4;
        const int dq = D / 4;
        for (int64_t i = start; i < total; i += step) {
            const int c = (int)(i % dq) * 4;
            float4 v = *reinterpret_cast<const float4*>(zr + 4 * i);
            const float4 A = *reinterpret_cast<const float4*>(ab + c), B = *reinterpret_cast<const float4*>(ab + D + c);
            v.x = __builtin_fmaf(v.x, A.x, B.x);
            v.y = __builtin_fmaf(v.y, A.y, B.y);
            v.z = __builtin_fmaf(v.z, A.z, B.z);
            v.w = __builtin_fmaf(v.w, A.w, B.w);
            *reinterpret_cast<float4*>(zr + 4 * i) = v;
        }
    } else {
        const int64_t total = N * D;
        for (int64_t i = start; i < total; i += step) {
            const int c = (int)(i % D);
            zr[i] = __builtin_fmaf(zr[i], ab[c], ab[D + c]);
        }
    }
    const float c0 = ldc[mp];
    float* sr = sld + m * N;
    for (int64_t i = start; i < N; i += step) sr[i] += c0;
}

// workspace of the forward, described once: moments [sum | sum of squares | unused] doubles | fold (Mp, 2, D) | ldc (Mp)
struct ArBatchFwdWs {
    double* moments;
    float *fold, *ldc;
    int64_t bytes;
};
static ArBatchFwdWs ar_batch_fwd_ws(int64_t Mp, int D, void* ws) {
    Carver c(ws);
    ArBatchFwdWs w = {};
    w.moments = c.take<double>(2 * (int64_t)D + 1, 16);
    w.fold = c.take<float>(Mp * 2 * D, 16);
    w.ldc = c.take<float>(Mp, 4);
    w.bytes = c.bytes(16);
    return w;
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// the slices of pass 1: BX workgroups per context, each a contiguous run of that context's rows.  A function of the shape
// alone, so the order of every addition is fixed.
static int64_t ar_batch_bwd_bx(int64_t M, int64_t N, int D) {
    const int64_t rpi = 256 / D;                          // rows per iteration of a workgroup (D <= 32)
    int64_t bx = (N + 16 * rpi - 1) / (16 * rpi);         // 16 iterations per workgroup ...
    const int64_t cap = 1024 / M < 1 ? 1 : 1024 / M;      // ... and about 1024 workgroups at most
    if (bx > cap) bx = cap;
    return bx < 1 ? 1 : bx;
}

// Pass 1.  Workgroup (bx, m): rows [bx rpb, (bx + 1) rpb) of context m; thread (r, d) adds rows r, r + rpi, ... of column d
// in double, the rpi row lanes are added in lane order -> part[(m BX + bx)][GZ (D) | GB (D) | GS]
__global__ void __launch_bounds__(256)
ar_batch_bwd_sums_kernel(const float* __restrict__ z, const float* __restrict__ g_z, const float* __restrict__ g_sld,
                         double* __restrict__ part, int64_t M, int64_t N, int D, int64_t rpb) {
    extern __shared__ double sred[];  // [rpi][2 D + 1]
    const int C = 2 * D + 1;
    const int rpi = 256 / D;
    const int tid = threadIdx.x;
    const int r = tid / D, d = tid - r * D;
    const int64_t m = grid_m();
    if (m >= M) return;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    int64_t r1 = r0 + rpb;
    if (r1 > N) r1 = N;
    if (r < rpi) {
        double gz = 0.0, gb = 0.0, gs = 0.0;
        const float* zc = z + m * N * D + d;
        const float* gc = g_z ? g_z + m * N * D + d : nullptr;
        const float* sc = (g_sld && d == 0) ? g_sld + m * N : nullptr;
        for (int64_t row = r0 + r; row < r1; row += rpi) {
            if (gc) {
                const double g = (double)gc[row * D];
                gz = fma(g, (double)zc[row * D], gz);
                gb += g;
            }
            if (sc) gs += (double)sc[row];
        }
        sred[r * C + d] = gz;
        sred[r * C + D + d] = gb;
        if (d == 0) sred[r * C + 2 * D] = gs;
    }
    __syncthreads();
    double* out = part + (m * gridDim.x + blockIdx.x) * C;
    for (int c = tid; c < C; c += 256) {
        double a = 0.0;
        for (int rr = 0; rr < rpi; ++rr) a += sred[rr * C + c];
        out[c] = a;
    }
}

// Pass 2, one workgroup of 1024 threads = S slices x C columns.  Slice s adds rows [s per, (s + 1) per) of part in row
// order; the slices are added in slice order.  -> glob = [P (D) | Q (D) | G | TZ (D) | TB (D) | TS]: P = sum e^a GB,
// Q = sum (GZ - b GB), G = sum GS over every context, and the plain totals of GZ | GB | GS (the sums of one shared row).
__global__ void __launch_bounds__(1024)
ar_batch_bwd_combine_kernel(const double* __restrict__ part, const float* __restrict__ params, int64_t pstride, int64_t p_maf,
                            int64_t Mp, int64_t rows, int64_t BX, double* __restrict__ glob, int D) {
    extern __shared__ double cred[];  // [S][C][2]
    const int C = 2 * D + 1;
    const int S = 1024 / C;
    const int tid = threadIdx.x;
    const int s = tid / C, c = tid - s * C;
    if (s < S) {
        const int64_t per = (rows + S - 1) / S;
        const int64_t i0 = (int64_t)s * per;
        int64_t i1 = i0 + per;
        if (i1 > rows) i1 = rows;
        double tot = 0.0, wsum = 0.0;  // wsum: e^a GB in a GB column, b GB in a GZ column (read from the GB column)
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t mp = Mp == 1 ? 0 : (int64_t)((int)i / (int)BX);
            const float* ap = params + mp * pstride + p_maf;
            tot += part[i * C + c];
            if (c < D) wsum = fma((double)ap[D + c], part[i * C + D + c], wsum);
            else if (c < 2 * D) wsum = fma(exp((double)ap[c - D]), part[i * C + c], wsum);
        }
        cred[(s * C + c) * 2] = tot;
        cred[(s * C + c) * 2 + 1] = wsum;
    }
    __syncthreads();
    if (tid < C) {
        double tot = 0.0, wsum = 0.0;
        for (int ss = 0; ss < S; ++ss) {
            tot += cred[(ss * C + tid) * 2];
            wsum += cred[(ss * C + tid) * 2 + 1];
        }
        glob[C + tid] = tot;
        if (tid < D) glob[D + tid] = tot - wsum;       // Q
        else if (tid < 2 * D) glob[tid - D] = wsum;    // P
        else glob[2 * D] = tot;                        // G
    }
}

// Pass 3, one workgroup per parameter row: the Affine gradient is added to its slice, the five coefficient rows written
__global__ void __launch_bounds__(64)
ar_batch_bwd_finalize_kernel(const double* __restrict__ part, const double* __restrict__ glob,
                             const float* __restrict__ params, int64_t pstride, int64_t p_maf,
                             const float* __restrict__ bn_mean, const float* __restrict__ bn_alpha,
                             float* __restrict__ g_params, int64_t gpstride, float* __restrict__ coef, int64_t Mp, int64_t BX,
                             double n, int D) {
    const int C = 2 * D + 1;
    const int64_t m = blockIdx.x;
    const float* ap = params + m * pstride + p_maf;
    float* gp = g_params + m * gpstride + p_maf;
    float* co = coef + m * 5 * D;
    const double G = glob[2 * D];
    for (int d = threadIdx.x; d < D; d += 64) {
        double GZ, GB, GS;
        if (Mp == 1) {
            GZ = glob[C + d];
            GB = glob[C + D + d];
            GS = glob[C + 2 * D];
        } else {
            GZ = GB = GS = 0.0;
            for (int64_t b = 0; b < BX; ++b) {
                const double* p = part + (m * BX + b) * C;
                GZ += p[d];
                GB += p[D + d];
                GS += p[2 * D];
            }
        }
        const double a = (double)ap[d], sh = (double)ap[D + d], al = (double)bn_alpha[d], mu = (double)bn_mean[d];
        gp[d] += (float)(GZ - sh * GB + GS);
        gp[D + d] += (float)GB;
        const double ea = exp(a), ia = exp(-a);
        const double A = al * ia;
        const double c2 = -ia * (glob[D + d] + G) / (n * al);
        co[d] = (float)A;
        co[D + d] = (float)(mu - sh * A);
        co[2 * D + d] = (float)(ea / al);
        co[3 * D + d] = (float)(-glob[d] / (n * al) - sh * c2);
        co[4 * D + d] = (float)c2;
    }
}

// workspace of the backward, described once: part (M BX, 2 D + 1) doubles | glob (2 (2 D + 1)) doubles | coef (Mp, 5, D)
struct ArBatchBwdWs {
    double *part, *glob;
    float* coef;
    int64_t BX, bytes;
};
static ArBatchBwdWs ar_batch_bwd_ws(int64_t M, int64_t Mp, int64_t N, int D, void* ws) {
    Carver c(ws);
    ArBatchBwdWs w = {};
    w.BX = ar_batch_bwd_bx(M, N, D);
    w.part = c.take<double>(M * w.BX * (2 * (int64_t)D + 1), 16);
    w.glob = c.take<double>(2 * (2 * (int64_t)D + 1), 8);
    w.coef = c.take<float>(Mp * 5 * D, 16);
    w.bytes = c.bytes(16);
    return w;
}

static int arbatch_mn(const char* fn, int64_t M, int64_t Mp, int64_t N) {
    if (M < 1 || (Mp != 1 && Mp != M) || N < 0)
        return fail(TNF_EINVAL, "%s: M=%lld M_p=%lld N=%lld", fn, (long long)M, (long long)Mp, (long long)N);
    return TNF_OK;
}

// the refusals the two calls share after their pointer checks; TNF_OK: the shape runs
static int arbatch_check(const char* fn, bool train, int64_t M, int64_t Mp, int64_t N, int D, int L, int U, int64_t pstride,
                         int64_t gpstride, const void* ws, int64_t ws_bytes, int64_t need_ws) {
    if (int rc = arbatch_mn(fn, M, Mp, N)) return rc;
    if (!(train ? tnf_ar_flow_batch_train_supported(D, L, U) : tnf_ar_flow_batch_supported(D, L, U)))
        return fail(TNF_EUNSUPPORTED, "%s: no kernel for D=%d L=%d U=%d", fn, D, L, U);
    const int64_t need = tnf_maf_num_params(D, L, U) + 2 * (int64_t)D;
    if (pstride < need || gpstride < need)
        return fail(TNF_EINVAL, "%s: parameter rows shorter than %lld", fn, (long long)need);
    if (N > 0 && M * N < 2) return fail(TNF_EINVAL, "%s: batch statistics need more than one row", fn);
    if (int rc = check_workspace(fn, ws, ws_bytes, need_ws, 16)) return rc;
    return TNF_OK;
}

}  // namespace tnf

using namespace tnf;

extern "C" {

int tnf_ar_flow_batch_supported(int32_t D, int32_t L, int32_t U) { return tnf_ar_flow_supported(D, L, U); }

int tnf_ar_flow_batch_train_supported(int32_t D, int32_t L, int32_t U) {
    return (tnf_ar_flow_supported(D, L, U) && maf_bwd_mfma_supported(D, L, U)) ? 1 : 0;
}

int64_t tnf_arbatch_launch_count(int32_t which) {
    if (which < 0 || which >= TNF_ARBATCH_COUNTERS) return fail(TNF_EINVAL, "tnf_arbatch_launch_count: counter %d", which);
    return g_arbatch_counts[which].load(std::memory_order_relaxed);
}

int64_t tnf_ar_flow_forward_batch_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D) {
    if (int rc = arbatch_mn("tnf_ar_flow_forward_batch_workspace_bytes", M, M_p, N)) return rc;
    if (D < 1) return fail(TNF_EINVAL, "tnf_ar_flow_forward_batch_workspace_bytes: D=%d", D);
    return ar_batch_fwd_ws(M_p, D, nullptr).bytes;
}

int tnf_ar_flow_forward_batch_f32(const float* omega, const float* params, const float* masks, float* z_out,
                                  float* sum_log_det, float* bn_mean_out, float* bn_alpha_out, int64_t M, int64_t M_p,
                                  int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, float eps, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_ar_flow_forward_batch_f32";
    if (!omega || !params || !masks || !z_out || !sum_log_det || !bn_mean_out || !bn_alpha_out)
        return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (z_out == omega) return fail(TNF_EINVAL, "%s: z_out must not alias omega", fn);
    if (int rc = arbatch_mn(fn, M, M_p, N)) return rc;
    const int64_t need_ws = D >= 1 ? ar_batch_fwd_ws(M_p, D, nullptr).bytes : 0;
    if (int rc = arbatch_check(fn, false, M, M_p, N, D, L, U, pstride, pstride, workspace, workspace_bytes, need_ws)) return rc;
    if (N == 0) return TNF_OK;
    const ArBatchFwdWs w = ar_batch_fwd_ws(M_p, D, workspace);
    hipStream_t st = as_stream(stream);
    const int64_t p_maf = tnf_maf_num_params(D, L, U);
    MafArgs a = {};
    a.z = omega; a.z_out = z_out; a.params = params; a.masks = masks; a.pstride = pstride;
    a.ld_out = sum_log_det; a.ld_sign = 1.f;
    a.Mz = M; a.Mp = M_p; a.N = N; a.D = D; a.L = L; a.U = U; a.inverse = 0;
    if (int rc = launch_maf_mfma(a, st)) return rc;
    if (int rc = launch_bn_moment_sums(z_out, w.moments, M * N, D, st)) return rc;
    hipLaunchKernelGGL(ar_batch_finalize_fold_kernel, dim3((unsigned)M_p), dim3(256), 0, st, params, pstride, p_maf,
                       (const double*)w.moments, (double)(M * N), eps, bn_mean_out, bn_alpha_out, w.fold, w.ldc, D);
    const int64_t per = (D % 4) == 0 && is_aligned(z_out, 16) ? N * D / 4 : N * D;
    const dim3 grid = grid_xm(persistent_bx(per, 1024, 2048, M), M);
    if ((D % 4) == 0 && is_aligned(z_out, 16))
        hipLaunchKernelGGL(ar_batch_apply_kernel<true>, grid, dim3(256), 0, st, z_out, sum_log_det, (const float*)w.fold,
                           (const float*)w.ldc, M, M_p, N, D);
    else
        hipLaunchKernelGGL(ar_batch_apply_kernel<false>, grid, dim3(256), 0, st, z_out, sum_log_det, (const float*)w.fold,
                           (const float*)w.ldc, M, M_p, N, D);
    if (int rc = check_launch(fn)) return rc;
    arbatch_count(TNF_ARBATCH_COUNT_FWD_CALLS, 1);
    arbatch_count(TNF_ARBATCH_COUNT_FWD_KERNELS, 4);
    return TNF_OK;
}

int64_t tnf_ar_flow_batch_bwd_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D) {
    if (int rc = arbatch_mn("tnf_ar_flow_batch_bwd_workspace_bytes", M, M_p, N)) return rc;
    if (D < 1 || D > 32) return fail(TNF_EINVAL, "tnf_ar_flow_batch_bwd_workspace_bytes: D=%d", D);
    return ar_batch_bwd_ws(M, M_p, N, D, nullptr).bytes;
}

int tnf_ar_flow_batch_bwd_f32(const float* z, const float* params, const float* masks, const float* bn_mean,
                              const float* bn_alpha, const float* g_z, const float* g_sld, float* g_params, int64_t M,
                              int64_t M_p, int64_t N, int32_t D, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tnf_ar_flow_batch_bwd_f32";
    if (!z || !params || !masks || !bn_mean || !bn_alpha || !g_params) return fail(TNF_EINVAL, "%s: NULL pointer", fn);
    if (!g_z && !g_sld) return fail(TNF_EINVAL, "%s: g_z and g_sld are both NULL", fn);
    if (g_params == params) return fail(TNF_EINVAL, "%s: g_params must not alias params", fn);
    if (int rc = arbatch_mn(fn, M, M_p, N)) return rc;
    const int64_t need_ws = (D >= 1 && D <= 32) ? ar_batch_bwd_ws(M, M_p, N, D, nullptr).bytes : 0;
    if (int rc = arbatch_check(fn, true, M, M_p, N, D, L, U, pstride, gpstride, workspace, workspace_bytes, need_ws)) return rc;
    if (N == 0) return TNF_OK;
    const ArBatchBwdWs w = ar_batch_bwd_ws(M, M_p, N, D, workspace);
    hipStream_t st = as_stream(stream);
    const int64_t p_maf = tnf_maf_num_params(D, L, U);
    const int C = 2 * D + 1, rpi = 256 / D;
    const int64_t rpb = (N + w.BX - 1) / w.BX;
    hipLaunchKernelGGL(ar_batch_bwd_sums_kernel, grid_xm(w.BX, M), dim3(256), (size_t)rpi * C * sizeof(double), st, z, g_z,
                       g_sld, w.part, M, N, D, rpb);
    hipLaunchKernelGGL(ar_batch_bwd_combine_kernel, dim3(1), dim3(1024), (size_t)(1024 / C) * C * 2 * sizeof(double), st,
                       (const double*)w.part, params, pstride, p_maf, M_p, M * w.BX, w.BX, w.glob, D);
    hipLaunchKernelGGL(ar_batch_bwd_finalize_kernel, dim3((unsigned)M_p), dim3(64), 0, st, (const double*)w.part,
                       (const double*)w.glob, params, pstride, p_maf, bn_mean, bn_alpha, g_params, gpstride, w.coef, M_p, w.BX,
                       (double)(M * N), D);
    if (int rc = check_launch(fn)) return rc;
    if (int rc = launch_maf_sample_bwd_batch(z, params, masks, g_z, g_sld, w.coef, g_params, M, M_p, N, D, L, U, pstride,
                                             gpstride, st))
        return rc;
    if (int rc = check_launch(fn)) return rc;
    arbatch_count(TNF_ARBATCH_COUNT_BWD_CALLS, 1);
    arbatch_count(TNF_ARBATCH_COUNT_BWD_KERNELS, 4);
    return TNF_OK;
}

}  // extern "C"
