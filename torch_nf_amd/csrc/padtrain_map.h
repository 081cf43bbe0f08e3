// The embedded layout of include/tnf_padtrain.h as index arithmetic: a coupling flow of width D inside one of width
// 2H.  Plain C++ (host and device): the kernels of flow_pad_train.hip use it, tnf_flow_padded_embed_index exports it.
#pragma once
#include "tnf_common.h"

namespace tnf {

__host__ __device__ inline int padtrain_half(int D) { return D >= 2 && D <= 31 ? 16 : (D >= 33 && D <= 63 ? 32 : 0); }

// real feature -> embedded feature, and back (-1: padding); the split of flow_fused2.hip's pad_feature
__host__ __device__ inline int padtrain_feature(int f, int H, int D) {
    const int h = D / 2;
    return f < h ? f : H + (f - h);
}
__host__ __device__ inline int padtrain_feature_real(int pf, int H, int D) {
    const int h = D / 2;
    if (pf < H) return pf < h ? pf : -1;
    return pf - H < D - h ? h + pf - H : -1;
}

// index r inside one RealNVP block of width D -> its index inside the block of width 2H
__host__ __device__ inline int64_t padtrain_coupling_index(int64_t r, int D, int H, int L, int U, int upper) {
    const CouplingDims c = coupling_dims(D, upper);
    const int64_t w0 = (int64_t)c.d_in * U;  // first layer: rows >= d_in are padding, so a weight keeps its offset
    if (r < 2 * w0) return (r / w0) * ((int64_t)H * U) + r % w0;
    r -= 2 * w0;
    int64_t off = 2 * (int64_t)H * U;
    const int64_t mid = 2 * (int64_t)U + (int64_t)(L - 1) * 2 * ((int64_t)U * U + U);  // its biases, the hidden layers
    if (r < mid) return off + r;
    r -= mid;
    off += mid;
    const int64_t w1 = (int64_t)U * c.d_out;  // last layer: columns >= d_out are padding
    if (r < 2 * w1) {
        const int64_t e = r % w1;
        return off + (r / w1) * ((int64_t)U * H) + (e / c.d_out) * H + e % c.d_out;
    }
    r -= 2 * w1;
    return off + 2 * (int64_t)U * H + (r / c.d_out) * H + r % c.d_out;
}

// THE index map: real index k of a (D, S, L, U) row -> index in the (2H, S, L, U) row.  Strictly increasing in k.
// The caller has checked 0 <= k < flow_layout(D, S, L, U).total and H = padtrain_half(D) != 0.
__host__ __device__ inline int64_t padtrain_embed_index(int64_t k, int D, int H, int L, int U, const FlowLayout& fr,
                                                        const FlowLayout& fe) {
    const int64_t base = (k / fr.stage) * fe.stage;
    int64_t r = k % fr.stage;
    if (r < fr.p_up) return base + padtrain_coupling_index(r, D, H, L, U, 1);
    r -= fr.p_up;
    if (r < fr.p_low) return base + fe.p_up + padtrain_coupling_index(r, D, H, L, U, 0);
    r -= fr.p_low;  // Affine [alpha (D) | shift (D)]
    return base + fe.p_up + fe.p_low + (r / D) * (2 * H) + padtrain_feature((int)(r % D), H, D);
}

}  // namespace tnf
