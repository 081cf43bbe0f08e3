// Exponential families of an EFN objective (exponential_families.py:104-307 of the reference): the sufficient
// statistics T(z) and the contraction eta . T(z) that the loss mean(log_q - eta . T(z)) is made of.
//   MVN        T(z) = [z | z_i z_j, i <= j, row-major over the upper triangle]        D_eta = D + D(D+1)/2
//   Dirichlet  T(z) = [log(z + 1e-10) | sum_i log(z_i + 1e-10)]                       D_eta = D + 1
// T(z) forward / backward: streaming kernels, float and double, any D (the reference's API, :140-156, :253-270).
// eta . T(z): never forms T(z).  For MVN it is the quadratic form eta1 . z + sum_{i<=j} eta2[i,j] z_i z_j; the packed
// upper triangle of eta IS row-major, so row i of U is the contiguous run eta[D + off(i) ..], no unpacking needed.
//   fused float32 kernels, 1 <= D <= 64: one workgroup = one context m x a run of 128-sample tiles.  A tile is staged
//   through LDS so that every global access is coalesced; then one sample per lane, its row of z in registers (D is a
//   template parameter, the i <= j loops are fully unrolled), and eta[m] -- wave-uniform -- read through the scalar
//   cache straight into the FMAs' scalar operand.  Exactly D(D+1)/2 + D FMAs per sample, nothing below the diagonal.
//   generic kernels (double, or D > 64): one sample per lane, run-time loops, eta and z through the vector caches.
// g_eta = sum_n g[n] T(z[n]) is a parameter gradient and is reduced in a fixed order: every workgroup owns one partial
// row in the workspace, every entry of it is owned by one thread, and an ordered pass adds the rows (no float atomics).
#include "launch.h"

namespace tnf {

#define TNF_EF_EPS 1e-10
enum { EF_TILE = 128, EF_GETA_THREADS = 256, EF_GETA_ROWS = 64 };

template <typename T> struct EfM;
template <> struct EfM<float> {
    static __device__ __forceinline__ float log(float x) { return logf(x); }
    static __device__ __forceinline__ float mul(float a, float b) { return __fmul_rn(a, b); }
};
template <> struct EfM<double> {
    static __device__ __forceinline__ double log(double x) { return ::log(x); }
    static __device__ __forceinline__ double mul(double a, double b) { return __dmul_rn(a, b); }
};

// start of row i inside the packed upper triangle of a D x D matrix
__host__ __device__ __forceinline__ int64_t ef_tri_off(int64_t i, int64_t D) { return i * D - i * (i - 1) / 2; }

// packed index p (0 .. D(D+1)/2 - 1) -> (i, j), i <= j
__device__ __forceinline__ void ef_tri_decode(int64_t p, int D, int& i, int& j) {
    const double b = 2.0 * D + 1.0;
    int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    if (r < 0) r = 0;
    if (r > D - 1) r = D - 1;
    while (r + 1 < D && ef_tri_off(r + 1, D) <= p) ++r;
    while (r > 0 && ef_tri_off(r, D) > p) --r;
    i = (int)r;
    j = (int)(r + (p - ef_tri_off(r, D)));
}

// ---------------------------------------------------------------------------
// T(z), forward and backward: one thread per output element, 64-bit element offsets
// ---------------------------------------------------------------------------
template <typename T, int FAM>
__global__ void __launch_bounds__(256)
ef_suffstats_kernel(const T* __restrict__ z, T* __restrict__ out, int64_t rows, int D, int Deta) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * Deta) return;
    const int64_t row = idx / Deta;
    const int k = (int)(idx - row * Deta);
    const T* zr = z + row * D;
    T v;
    if (FAM == TNF_EF_MVN) {
        if (k < D) {
            v = zr[k];
        } else {
            int i, j;
            ef_tri_decode(k - D, D, i, j);
            v = EfM<T>::mul(zr[i], zr[j]);
        }
    } else {
        if (k < D) {
            v = EfM<T>::log(zr[k] + (T)TNF_EF_EPS);
        } else {
            v = 0;
            for (int d = 0; d < D; ++d) v += EfM<T>::log(zr[d] + (T)TNF_EF_EPS);
        }
    }
    out[idx] = v;
}

// MVN: g_z[i] = g_T[i] + sum_j g_T[idx(min(i,j), max(i,j))] z_j (1 + [i == j]);  Dirichlet: (g_T[i] + g_T[D]) / (z_i + eps)
template <typename T, int FAM>
__global__ void __launch_bounds__(256)
ef_suffstats_backward_kernel(const T* __restrict__ z, const T* __restrict__ g_T, T* __restrict__ g_z, int64_t rows, int D,
                             int Deta) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * D) return;
    const int64_t row = idx / D;
    const int i = (int)(idx - row * D);
    const T* zr = z + row * D;
    const T* gr = g_T + row * Deta;
    if (FAM == TNF_EF_MVN) {
        T acc = gr[i];
        for (int j = 0; j < D; ++j) {
            const int lo = j < i ? j : i, hi = j < i ? i : j;
            const T g = gr[D + ef_tri_off(lo, D) + (hi - lo)];
            acc += g * zr[j] * (i == j ? (T)2 : (T)1);
        }
        g_z[idx] = acc;
    } else {
        g_z[idx] = (gr[i] + gr[D]) / (zr[i] + (T)TNF_EF_EPS);
    }
}

// ---------------------------------------------------------------------------
// eta . T(z), fused float32, 1 <= D <= 64
// ---------------------------------------------------------------------------
// Stage rows [n0, n0 + nr) of one context into LDS, row stride LD (odd: a lane per row reads conflict-free).
__device__ __forceinline__ void ef_stage(float* tile, const float* __restrict__ src, int nr, int D, int LD, int tid) {
    for (int idx = tid; idx < nr * D; idx += EF_TILE) {
        const int r = idx / D, d = idx - r * D;
        tile[r * LD + d] = src[idx];
    }
}

template <int D>
__global__ void __launch_bounds__(EF_TILE)
ef_dot_mvn_kernel(const float* __restrict__ z, const float* __restrict__ eta, float* __restrict__ out, int64_t M, int64_t N,
                  int64_t ld_eta, int tiles_per_wg) {
    constexpr int LD = D | 1;
    __shared__ float tile[EF_TILE * LD];
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const float* __restrict__ e = eta + m * ld_eta;
    const float* zm = z + m * N * D;
    for (int t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * EF_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)EF_TILE ? (N - n0) : (int64_t)EF_TILE);
        __syncthreads();
        ef_stage(tile, zm + n0 * D, nr, D, LD, tid);
        __syncthreads();
        if (tid < nr) {
            float zr[D];
#pragma unroll
            for (int d = 0; d < D; ++d) zr[d] = tile[tid * LD + d];
            float acc = 0.0f;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int base = D + i * D - i * (i - 1) / 2 - i;  // eta2[i, j] = e[base + j]
                float r = e[i];
#pragma unroll
                for (int j = i; j < D; ++j) r = fmaf(e[base + j], zr[j], r);
                acc = fmaf(zr[i], r, acc);
            }
            out[m * N + n0 + tid] = acc;
        }
    }
}

// g_z[m,n,:] = g[m,n] * (eta1 + (U + U^T) z): each packed entry feeds the two rows it belongs to (the diagonal twice)
template <int D>
__global__ void __launch_bounds__(EF_TILE)
ef_dot_mvn_gz_kernel(const float* __restrict__ z, const float* __restrict__ eta, const float* __restrict__ g_out,
                     float* __restrict__ g_z, int64_t M, int64_t N, int64_t ld_eta, int tiles_per_wg) {
    constexpr int LD = D | 1;
    __shared__ float tile[EF_TILE * LD];
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const float* __restrict__ e = eta + m * ld_eta;
    const float* zm = z + m * N * D;
    float* gm = g_z + m * N * D;
    for (int t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * EF_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)EF_TILE ? (N - n0) : (int64_t)EF_TILE);
        __syncthreads();
        ef_stage(tile, zm + n0 * D, nr, D, LD, tid);
        __syncthreads();
        if (tid < nr) {
            float zr[D], a[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                zr[d] = tile[tid * LD + d];
                a[d] = e[d];
            }
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const int base = D + i * D - i * (i - 1) / 2 - i;
#pragma unroll
                for (int j = i; j < D; ++j) {
                    const float u = e[base + j];
                    a[i] = fmaf(u, zr[j], a[i]);
                    a[j] = fmaf(u, zr[i], a[j]);
                }
            }
            const float g = g_out[m * N + n0 + tid];
#pragma unroll
            for (int d = 0; d < D; ++d) tile[tid * LD + d] = g * a[d];  // the lane's own row: no other lane reads it
        }
        __syncthreads();
        for (int idx = tid; idx < nr * D; idx += EF_TILE) {
            const int r = idx / D, d = idx - r * D;
            gm[n0 * D + idx] = tile[r * LD + d];
        }
    }
}

// Dirichlet: out = sum_i (eta_i + eta_D) log(z_i + eps); run-time D <= 64, LDS row stride D | 1
__global__ void __launch_bounds__(EF_TILE)
ef_dot_dirichlet_kernel(const float* __restrict__ z, const float* __restrict__ eta, float* __restrict__ out, int64_t M,
                        int64_t N, int D, int64_t ld_eta, int tiles_per_wg) {
    __shared__ float tile[EF_TILE * 65];
    const int LD = D | 1;
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const float* __restrict__ e = eta + m * ld_eta;
    const float eD = e[D];
    const float* zm = z + m * N * D;
    for (int t = 0; t < tiles_per_wg; ++t) {
        const int64_t n0 = ((int64_t)blockIdx.x * tiles_per_wg + t) * EF_TILE;
        if (n0 >= N) break;
        const int nr = (int)((N - n0) < (int64_t)EF_TILE ? (N - n0) : (int64_t)EF_TILE);
        __syncthreads();
        ef_stage(tile, zm + n0 * D, nr, D, LD, tid);
        __syncthreads();
        if (tid < nr) {
            float acc = 0.0f;
            for (int d = 0; d < D; ++d) acc = fmaf(e[d] + eD, logf(tile[tid * LD + d] + (float)TNF_EF_EPS), acc);
            out[m * N + n0 + tid] = acc;
        }
    }
}

__global__ void __launch_bounds__(256)
ef_dot_dirichlet_gz_kernel(const float* __restrict__ z, const float* __restrict__ eta, const float* __restrict__ g_out,
                           float* __restrict__ g_z, int64_t M, int64_t N, int D, int64_t ld_eta) {
    const int64_t m = grid_m();
    if (m >= M) return;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // inside context m
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int d = (int)(idx - n * D);
    const float* e = eta + m * ld_eta;
    g_z[m * N * D + idx] = g_out[m * N + n] * (e[d] + e[D]) / (z[m * N * D + idx] + (float)TNF_EF_EPS);
}

// ---------------------------------------------------------------------------
// eta . T(z), shape-generic (double, or D > 64): one sample per lane
// ---------------------------------------------------------------------------
template <typename T, int FAM>
__global__ void __launch_bounds__(256)
ef_dot_generic_kernel(const T* __restrict__ z, const T* __restrict__ eta, T* __restrict__ out, int64_t M, int64_t N, int D,
                      int64_t ld_eta) {
    const int64_t m = grid_m();
    if (m >= M) return;
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const T* e = eta + m * ld_eta;
    const T* zr = z + (m * N + n) * D;
    T acc = 0;
    if (FAM == TNF_EF_MVN) {
        for (int i = 0; i < D; ++i) {
            const T* u = e + D + ef_tri_off(i, D) - i;
            T r = e[i];
            for (int j = i; j < D; ++j) r += u[j] * zr[j];
            acc += zr[i] * r;
        }
    } else {
        const T eD = e[D];
        for (int d = 0; d < D; ++d) acc += (e[d] + eD) * EfM<T>::log(zr[d] + (T)TNF_EF_EPS);
    }
    out[m * N + n] = acc;
}

template <typename T, int FAM>
__global__ void __launch_bounds__(256)
ef_dot_generic_gz_kernel(const T* __restrict__ z, const T* __restrict__ eta, const T* __restrict__ g_out,
                         T* __restrict__ g_z, int64_t M, int64_t N, int D, int64_t ld_eta) {
    const int64_t m = grid_m();
    if (m >= M) return;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * D) return;
    const int64_t n = idx / D;
    const int i = (int)(idx - n * D);
    const T* e = eta + m * ld_eta;
    const T* zr = z + (m * N + n) * D;
    const T g = g_out[m * N + n];
    if (FAM == TNF_EF_MVN) {
        T acc = e[i];
        for (int j = 0; j < D; ++j) {
            const int lo = j < i ? j : i, hi = j < i ? i : j;
            acc += e[D + ef_tri_off(lo, D) + (hi - lo)] * zr[j] * (i == j ? (T)2 : (T)1);
        }
        g_z[m * N * D + idx] = g * acc;
    } else {
        g_z[m * N * D + idx] = g * (e[i] + e[D]) / (zr[i] + (T)TNF_EF_EPS);
    }
}

// ---------------------------------------------------------------------------
// g_eta[m,:] = sum_n g[m,n] T(z[m,n]), bit-reproducible
// ---------------------------------------------------------------------------
// Workgroup (chunk c, context m) walks its tiles of R samples in order and owns partial row (m, c) of the workspace;
// thread t owns entries t, t + 256, ... of that row and adds each tile's sum (taken in sample order) to them.
template <typename T, int FAM>
__global__ void __launch_bounds__(EF_GETA_THREADS)
ef_geta_partial_kernel(const T* __restrict__ z, const T* __restrict__ g_out, T* __restrict__ partial, int64_t M, int64_t N,
                       int D, int Deta, int G, int R, int64_t tiles_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    T* tile = reinterpret_cast<T*>(smem_raw);  // [R][D]: z (MVN) or log(z + eps) (Dirichlet)
    T* gs = tile + (int64_t)R * D;             // [R]
    const int64_t m = grid_m();
    if (m >= M) return;
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    T* row = partial + (m * G + c) * (int64_t)Deta;
    const int64_t ntiles = (N + R - 1) / R;
    const int64_t t0 = (int64_t)c * tiles_per_chunk;
    int64_t t1 = t0 + tiles_per_chunk;
    if (t1 > ntiles) t1 = ntiles;
    bool first = true;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t n0 = t * R;
        const int nr = (int)((N - n0) < (int64_t)R ? (N - n0) : (int64_t)R);
        __syncthreads();
        const T* zt = z + (m * N + n0) * D;
        for (int idx = tid; idx < nr * D; idx += EF_GETA_THREADS)
            tile[idx] = FAM == TNF_EF_MVN ? zt[idx] : EfM<T>::log(zt[idx] + (T)TNF_EF_EPS);
        for (int s = tid; s < nr; s += EF_GETA_THREADS) gs[s] = g_out[m * N + n0 + s];
        __syncthreads();
        for (int k = tid; k < Deta; k += EF_GETA_THREADS) {
            T acc = 0;  // the tile's own sum first, then one add into the running row: shorter error chains
            if (FAM == TNF_EF_MVN) {
                if (k < D) {
                    for (int s = 0; s < nr; ++s) acc += gs[s] * tile[s * D + k];
                } else {
                    int i, j;
                    ef_tri_decode(k - D, D, i, j);
                    for (int s = 0; s < nr; ++s) acc += gs[s] * (tile[s * D + i] * tile[s * D + j]);
                }
            } else {
                if (k < D) {
                    for (int s = 0; s < nr; ++s) acc += gs[s] * tile[s * D + k];
                } else {
                    for (int s = 0; s < nr; ++s) {
                        T h = 0;
                        for (int d = 0; d < D; ++d) h += tile[s * D + d];
                        acc += gs[s] * h;
                    }
                }
            }
            row[k] = first ? acc : row[k] + acc;
        }
        first = false;
    }
    if (first)
        for (int k = tid; k < Deta; k += EF_GETA_THREADS) row[k] = (T)0;
}

template <typename T>
__global__ void __launch_bounds__(256)
ef_geta_reduce_kernel(const T* __restrict__ partial, T* __restrict__ g_eta, int64_t M, int Deta, int G) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * Deta) return;
    const int64_t m = idx / Deta;
    const int k = (int)(idx - m * Deta);
    T acc = 0;
    for (int c = 0; c < G; ++c) acc += partial[(m * G + c) * (int64_t)Deta + k];
    g_eta[idx] = acc;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int64_t ef_num_eta(int family, int D) {
    if (D < 1 || D > TNF_EF_MAX_D) return -1;
    if (family == TNF_EF_MVN) return (int64_t)D + (int64_t)D * (D + 1) / 2;
    if (family == TNF_EF_DIRICHLET) return (int64_t)D + 1;
    return -1;
}

bool ef_dot_fused_supported(int family, int D) {
    return (family == TNF_EF_MVN || family == TNF_EF_DIRICHLET) && D >= 1 && D <= 64;
}

static int ef_geta_rows(int D) {  // samples per staged tile of the g_eta kernel: 48 KB of doubles at the most
    int64_t R = (int64_t)(48 * 1024) / ((int64_t)(D + 1) * 8);
    if (R > EF_GETA_ROWS) R = EF_GETA_ROWS;
    return (int)R;  // 0: D too large
}

static int ef_geta_chunks(int64_t M, int64_t N, int D) {
    const int R = ef_geta_rows(D);
    if (R < 1) return -1;
    int64_t G = (N + R - 1) / R;
    const int64_t cap = M >= 256 ? 1 : 256 / M;
    if (G > cap) G = cap;
    if (G < 1) G = 1;
    return (int)G;
}

int64_t ef_dot_bwd_workspace(int family, int64_t M, int64_t N, int D) {
    const int64_t Deta = ef_num_eta(family, D);
    const int G = ef_geta_chunks(M, N, D);
    if (Deta < 0 || G < 0) return -1;
    return M * G * Deta * 8;
}

// (dtype, family) -> <T, FAM> of the dtype-generic kernels: f(T{}, int_c<FAM>{})
template <class F> static auto dispatch_ef(int dtype, int family, F&& f) {
    return dispatch_dtype(dtype, [&](auto t) {
        return family == TNF_EF_MVN ? f(t, int_c<TNF_EF_MVN>{}) : f(t, int_c<TNF_EF_DIRICHLET>{});
    });
}

int launch_ef_suffstats(int dtype, int family, const void* z, void* out, int64_t rows, int D, hipStream_t st) {
    if (rows == 0) return 0;
    const int Deta = (int)ef_num_eta(family, D);
    const int64_t blocks = (rows * Deta + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "ef_suffstats: grid too large");
    dispatch_ef(dtype, family, [&](auto t, auto fam) {
        using T = decltype(t);
        hipLaunchKernelGGL((ef_suffstats_kernel<T, fam()>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)z, (T*)out,
                           rows, D, Deta);
    });
    return check_launch("ef_suffstats");
}

int launch_ef_suffstats_backward(int dtype, int family, const void* z, const void* g_T, void* g_z, int64_t rows, int D,
                                 hipStream_t st) {
    if (rows == 0) return 0;
    const int Deta = (int)ef_num_eta(family, D);
    const int64_t blocks = (rows * D + 255) / 256;
    if (blocks > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "ef_suffstats_backward: grid too large");
    dispatch_ef(dtype, family, [&](auto t, auto fam) {
        using T = decltype(t);
        hipLaunchKernelGGL((ef_suffstats_backward_kernel<T, fam()>), dim3((unsigned)blocks), dim3(256), 0, st, (const T*)z,
                           (const T*)g_T, (T*)g_z, rows, D, Deta);
    });
    return check_launch("ef_suffstats_backward");
}

// a workgroup of the fused kernels walks a run of tiles: enough workgroups to fill the device several times over, and
// no more (eta[m] is fetched once per tile through the scalar cache; the run only bounds the grid)
static int ef_tiles_per_wg(int64_t M, int64_t N, int64_t* bx) {
    const int64_t tiles = (N + EF_TILE - 1) / EF_TILE;
    int64_t want = 8192 / (M < 8192 ? M : 8192);  // workgroups per context
    if (want < 1) want = 1;
    int64_t per = (tiles + want - 1) / want;
    if (per < 1) per = 1;
    if (per > 64) per = 64;
    *bx = (tiles + per - 1) / per;
    return (int)per;
}

#define TNF_EF_CASE(Dv, KERNEL, ...)                                                                              \
    case Dv:                                                                                                      \
        hipLaunchKernelGGL((KERNEL<Dv>), grid, dim3(EF_TILE), 0, st, __VA_ARGS__);                                \
        break;
#define TNF_EF_CASES8(B, KERNEL, ...)                                                                             \
    TNF_EF_CASE(B + 1, KERNEL, __VA_ARGS__) TNF_EF_CASE(B + 2, KERNEL, __VA_ARGS__)                               \
    TNF_EF_CASE(B + 3, KERNEL, __VA_ARGS__) TNF_EF_CASE(B + 4, KERNEL, __VA_ARGS__)                               \
    TNF_EF_CASE(B + 5, KERNEL, __VA_ARGS__) TNF_EF_CASE(B + 6, KERNEL, __VA_ARGS__)                               \
    TNF_EF_CASE(B + 7, KERNEL, __VA_ARGS__) TNF_EF_CASE(B + 8, KERNEL, __VA_ARGS__)
#define TNF_EF_SWITCH(KERNEL, ...)                                                                                \
    switch (D) {                                                                                                  \
        TNF_EF_CASES8(0, KERNEL, __VA_ARGS__) TNF_EF_CASES8(8, KERNEL, __VA_ARGS__)                               \
        TNF_EF_CASES8(16, KERNEL, __VA_ARGS__) TNF_EF_CASES8(24, KERNEL, __VA_ARGS__)                             \
        TNF_EF_CASES8(32, KERNEL, __VA_ARGS__) TNF_EF_CASES8(40, KERNEL, __VA_ARGS__)                             \
        TNF_EF_CASES8(48, KERNEL, __VA_ARGS__) TNF_EF_CASES8(56, KERNEL, __VA_ARGS__)                             \
        default:                                                                                                  \
            return fail(TNF_EUNSUPPORTED, "ef_dot: no fused kernel for D=%d", D);                                 \
    }

int launch_ef_dot(int dtype, int family, const void* z, const void* eta, void* out, int64_t M, int64_t N, int D,
                  int64_t ld_eta, hipStream_t st) {
    if (M == 0 || N == 0) return 0;
    if ((N * D + 255) / 256 > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "ef_dot: grid too large");
    if (dtype == TNF_F32 && !g_force_generic && ef_dot_fused_supported(family, D)) {
        int64_t bx;
        const int per = ef_tiles_per_wg(M, N, &bx);
        const dim3 grid = grid_xm(bx, M);
        if (family == TNF_EF_MVN) {
            TNF_EF_SWITCH(ef_dot_mvn_kernel, (const float*)z, (const float*)eta, (float*)out, M, N, ld_eta, per)
        } else {
            hipLaunchKernelGGL(ef_dot_dirichlet_kernel, grid, dim3(EF_TILE), 0, st, (const float*)z, (const float*)eta,
                               (float*)out, M, N, D, ld_eta, per);
        }
        ef_count(TNF_EF_COUNT_DOT);
        return check_launch("ef_dot");
    }
    dispatch_ef(dtype, family, [&](auto t, auto fam) {
        using T = decltype(t);
        hipLaunchKernelGGL((ef_dot_generic_kernel<T, fam()>), grid_xm((N + 255) / 256, M), dim3(256), 0, st, (const T*)z,
                           (const T*)eta, (T*)out, M, N, D, ld_eta);
    });
    return check_launch("ef_dot (generic)");
}

template <typename T, int FAM>
static int ef_launch_geta(const void* z, const void* g, void* g_eta, int64_t M, int64_t N, int D, int Deta, void* ws,
                          hipStream_t st) {
    const int R = ef_geta_rows(D);
    const int G = ef_geta_chunks(M, N, D);
    const int64_t ntiles = (N + R - 1) / R;
    const int64_t per = ntiles > 0 ? (ntiles + G - 1) / G : 1;
    const size_t smem = ((size_t)R * D + R) * sizeof(T);
    int rc = launch_lds("ef_dot_backward", ef_geta_partial_kernel<T, FAM>, grid_xm(G, M), dim3(EF_GETA_THREADS), smem, st,
                        (const T*)z, (const T*)g, (T*)ws, M, N, D, Deta, G, R, per);
    if (rc) return rc;
    rc = check_launch("ef_dot_backward (g_eta partials)");
    if (rc) return rc;
    hipLaunchKernelGGL((ef_geta_reduce_kernel<T>), dim3((unsigned)((M * Deta + 255) / 256)), dim3(256), 0, st,
                       (const T*)ws, (T*)g_eta, M, Deta, G);
    return check_launch("ef_dot_backward (g_eta reduce)");
}

int launch_ef_dot_backward(int dtype, int family, const void* z, const void* eta, const void* g_out, void* g_z,
                           void* g_eta, int64_t M, int64_t N, int D, int64_t ld_eta, void* ws, hipStream_t st) {
    if (M == 0) return 0;
    if ((N * D + 255) / 256 > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "ef_dot_backward: grid too large");
    const int Deta = (int)ef_num_eta(family, D);
    if (g_z && N > 0) {
        if (dtype == TNF_F32 && !g_force_generic && ef_dot_fused_supported(family, D)) {
            if (family == TNF_EF_MVN) {
                int64_t bx;
                const int per = ef_tiles_per_wg(M, N, &bx);
                const dim3 grid = grid_xm(bx, M);
                TNF_EF_SWITCH(ef_dot_mvn_gz_kernel, (const float*)z, (const float*)eta, (const float*)g_out, (float*)g_z,
                              M, N, ld_eta, per)
            } else {
                hipLaunchKernelGGL(ef_dot_dirichlet_gz_kernel, grid_xm((N * D + 255) / 256, M), dim3(256), 0, st,
                                   (const float*)z, (const float*)eta, (const float*)g_out, (float*)g_z, M, N, D, ld_eta);
            }
            ef_count(TNF_EF_COUNT_DOT_BWD);
        } else {
            dispatch_ef(dtype, family, [&](auto t, auto fam) {
                using T = decltype(t);
                hipLaunchKernelGGL((ef_dot_generic_gz_kernel<T, fam()>), grid_xm((N * D + 255) / 256, M), dim3(256), 0, st,
                                   (const T*)z, (const T*)eta, (const T*)g_out, (T*)g_z, M, N, D, ld_eta);
            });
        }
        const int rc = check_launch("ef_dot_backward (g_z)");
        if (rc) return rc;
    }
    if (g_eta) {
        if ((M * Deta + 255) / 256 > 0x7fffffff) return fail(TNF_EUNSUPPORTED, "ef_dot_backward: grid too large");
        return dispatch_ef(dtype, family, [&](auto t, auto fam) {
            return ef_launch_geta<decltype(t), fam()>(z, g_out, g_eta, M, N, D, Deta, ws, st);
        });
    }
    return TNF_OK;
}

}  // namespace tnf
