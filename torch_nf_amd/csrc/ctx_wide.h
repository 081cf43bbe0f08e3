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

// The team size of a backward launch (flow_ctx_wide_bwd.hip, flow_ctx_wide_sample_bwd.hip; host code), measured at 4, 8
// and 16 waves (profiles/r22_ctxwidebench_waves.txt).  The
// widest steps of the walk are the weight-gradient contractions, 2 U U items (2 U ceil(D / 2) for the first and last
// layer): where they have at most 1,024 items (20 units below D = 64) four waves are 1.1 .. 1.3 x faster than eight, above
// that eight are 1.2 .. 1.5 x faster than four; sixteen win, 1.4 .. 1.5 x over eight, only in the one class where every
// step is wide -- two tiles of samples, more than 48 units and D >= 32 -- and lose 1.1 .. 1.8 x elsewhere.  33 .. 48
// units were not measured and follow the item count.  The results are the same bits for every team size.
inline int cwb_waves(int N, int D, int U) {
    if (N > 16 && U > 48 && D >= 32) return 16;
    const int widest = 2 * U * (U > (D + 1) / 2 ? U : (D + 1) / 2);
    return widest <= 1024 ? 4 : 8;
}

}  // namespace tnf
