// The domain, LDS needs and support predicates of the per-context kernels above 16 units (include/tnf_ctxwide.h):
// flow_ctx_wide.hip (inference, one layer's operand image of wide_flow_tile.h resident at a time) and
// flow_ctx_wide_bwd.hip (the log_prob backward on the walk of ctx_bwd_walk.h).  Restated by tests/test_ctx_wide_host.py.
#pragma once
#include "ctx_bwd_walk.h"
#include "wide_flow_tile.h"

namespace tnf {

constexpr int64_t kCtxWideLdsBudget = kWideFlowLdsBudget;  // 150 KB of the CU's 160

inline bool ctx_wide_domain(int D, int S, int U, int64_t N) {
    return D >= 2 && D <= 64 && S >= 1 && U >= 17 && U <= 64 && N >= 1 && N <= 31;
}
// dynamic LDS of one workgroup: which = 0 the inference launch (one layer's image and fold block), which = 1 the
// backward launch (one context's slice); -1 outside the domain
inline int64_t ctx_wide_lds_bytes(int which, int D, int S, int L, int U, int64_t N) {
    if (!ctx_wide_domain(D, S, U, N) || L < 1) return -1;
    if (which == 0) {  // wide_flow_layer_floats in 64 bits: any L
        const int64_t HT = ((D + 1) / 2 + 15) / 16, UT = (U + 15) / 16;
        return 4 * (256 * (4 * HT * UT + 2 * ((int64_t)L - 1) * UT * UT) + 16 * (2 * (int64_t)L * UT + 2 * HT) + 64 * HT);
    }
    if (which == 1) return 4 * ctx_bwd_slice_floats((int)N, D, S, L, U);
    return -1;
}
inline bool ctx_wide_supported(int D, int S, int L, int U, int64_t N) {
    return ctx_wide_domain(D, S, U, N) && L >= 1 && L <= 5 && ctx_wide_lds_bytes(0, D, S, L, U, N) <= kCtxWideLdsBudget;
}
inline bool ctx_wide_train_supported(int D, int S, int L, int U, int64_t N) {
    return ctx_wide_domain(D, S, U, N) && L >= 1 && L <= 3 && ctx_wide_lds_bytes(1, D, S, L, U, N) <= kCtxWideLdsBudget;
}

}  // namespace tnf
