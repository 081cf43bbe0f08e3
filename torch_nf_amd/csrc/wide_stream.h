// The streamed whole-flow form of the "wide" fp32-MFMA coupling tile (flow_wide_stream.hip, include/tnf_widestream.h):
// its support predicate, LDS sizes and tile rule in plain C++17 (no HIP), so that host tests restate them
// (tests/widestream_restatement.py).
//
// flow_wide.hip keeps the operand images of all 2 S coupling layers in LDS, which caps S (wide_flow_supported).  The
// streamed kernel keeps a ring of one or two layers -- wide_flow_layer_floats(D, L, U) floats each, image plus fold
// block -- and rebuilds the next layer while (two slots) or after (one slot) the workgroup computes the current one, so
// S is bounded only by the range of the walk's counters.
//     wide_stream_supported(D, S, L, U): 2 <= D <= 64, 1 <= S <= 1024, 1 <= L <= 5, 17 <= U <= 64 and
//                                        4 * wide_flow_layer_floats(D, L, U) <= 153,600 B
//     wide_stream_slots(D, L, U):        2 when two layers fit the budget, else 1 (0 outside the domain)
//     wide_stream_lds_bytes(D, L, U):    4 * slots * wide_flow_layer_floats(D, L, U)
//     (64, ., 2, 64): 67,328 B per layer, two slots, 134,656 B; (8, ., 5, 64): 150,400 B, one slot;
//     (64, ., 5, 64): 167,168 B, refused.
#pragma once
#include <type_traits>

#include "wide_flow_tile.h"

namespace tnf {

constexpr int WS_WAVES = 8;      // one workgroup per parameter row, as flow_wide.hip
constexpr int kWideStreamMaxS = 1024;

inline bool wide_stream_domain(int D, int L, int U) {
    if (D < 2 || D > 64 || L < 1 || L > 5 || U < 17 || U > 64) return false;
    return 4 * wide_flow_layer_floats(D, L, U) <= kWideFlowLdsBudget;
}
inline bool wide_stream_supported(int D, int S, int L, int U) {
    return S >= 1 && S <= kWideStreamMaxS && wide_stream_domain(D, L, U);
}
inline int wide_stream_slots(int D, int L, int U) {
    if (!wide_stream_domain(D, L, U)) return 0;
    return 8 * wide_flow_layer_floats(D, L, U) <= kWideFlowLdsBudget ? 2 : 1;
}
inline int64_t wide_stream_lds_bytes(int D, int L, int U) {
    return 4 * (int64_t)wide_stream_slots(D, L, U) * (wide_stream_domain(D, L, U) ? wide_flow_layer_floats(D, L, U) : 0);
}

// T, the 16-sample tiles a wave holds in registers: a workgroup walks groups of WS_WAVES * T tiles and rebuilds every
// layer's image once per group, so a larger T divides the rebuilds per sample by T.  The shipped values and the rule
// that picks among them: flow_wide_stream.hip (wide_stream_tiles).
inline int64_t wide_stream_groups(int64_t N, int T) {
    const int64_t ntiles = (N + 15) / 16;
    return (ntiles + WS_WAVES * T - 1) / (WS_WAVES * T);
}
inline bool wide_stream_tiles_shipped(int T) { return T == 1 || T == 2 || T == 4; }
// The largest T instantiated for a tile shape: 4, but at HT = 2 with UT = 4 (D >= 33, U >= 49) the layer body leaves
// room for T = 2 only, and with the refined activation (L >= 4) for T = 1: the larger ones spill
// (profiles/r24_widestream_resources.txt).  A forced T above it is clamped to it.
constexpr int wide_stream_max_tiles(int HT, int UT, bool deep) { return HT == 2 && UT == 4 ? (deep ? 1 : 2) : 4; }
// The rule: the largest T the shape has that (a) still leaves one group for each of the 256 CUs, M groups(N, T) >= 256
// -- a larger T on fewer groups would idle CUs to save rebuilds -- and (b) has tiles for the slots it adds,
// ceil(N / 16) > 8 (T / 2); else 1 (rows of about 100 samples: seven tiles, one group at any T).
inline int wide_stream_tiles(int D, int L, int U, int64_t M, int64_t N) {
    const WideLayout wl = wide_flow_layout(D, L, U);
    for (int T = wide_stream_max_tiles(wl.HT, wl.UT, L > 3); T > 1; T >>= 1)
        if (wide_stream_groups(N, T) >= (256 + M - 1) / M && (N + 15) / 16 > WS_WAVES * (T / 2)) return T;
    return 1;
}
template <class F> auto dispatch_wide_stream_tiles(int T, F&& f) {
    switch (T) {
        case 4: return f(std::integral_constant<int, 4>{});
        case 2: return f(std::integral_constant<int, 2>{});
        default: return f(std::integral_constant<int, 1>{});
    }
}

}  // namespace tnf
