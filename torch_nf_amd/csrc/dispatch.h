// Run-time value -> template argument, once.  Each helper calls `f` with the value as a compile-time tag and returns what
// `f` returns; they nest, so a launcher names its kernel in one place, inside the lambdas.  Plain C++17, no HIP: the
// mappings are checked on the CPU (tests/test_dispatch_host.py).  Support checks stay with the callers and come first.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/tnf.h"

namespace tnf {

template <int V> using int_c = std::integral_constant<int, V>;

// 1, 2, 3 and anything else -> 4 (tile counts HT / UT / DT; depth of the wide layouts)
template <class F> auto dispatch_1to4(int n, F&& f) {
    switch (n) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        case 3: return f(int_c<3>{});
        default: return f(int_c<4>{});
    }
}

// 1, 2 and anything else -> 3 (hidden layers of the D = 32 / 64 MFMA kernels)
template <class F> auto dispatch_1to3(int n, F&& f) {
    switch (n) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        default: return f(int_c<3>{});
    }
}

// (D, L) -> <H, L>: H = 32 for D == 64, 16 for anything else
template <class F> auto dispatch_hl(int D, int L, F&& f) {
    return dispatch_1to3(L, [&](auto l) { return D == 64 ? f(int_c<32>{}, l) : f(int_c<16>{}, l); });
}

template <class F> auto dispatch_bool(bool flag, F&& f) {
    return flag ? f(std::true_type{}) : f(std::false_type{});
}

// TNF_F32 -> float, anything else -> double
template <class F> auto dispatch_dtype(int dtype, F&& f) {
    return dtype == TNF_F32 ? f(float{}) : f(double{});
}

// LO .. HI, one case each (the caller has checked the range; anything above goes to HI)
template <int LO, int HI, class F> auto dispatch_range(int n, F&& f) {
    if constexpr (LO == HI) {
        return f(int_c<LO>{});
    } else {
        return n == LO ? f(int_c<LO>{}) : dispatch_range<LO + 1, HI>(n, f);
    }
}

// grid.x of a persistent kernel: one workgroup per `per_wg` items, at most budget / M (and at least one) per context.
// Pure arithmetic, kept here beside the dispatchers so that the CPU test reaches it without HIP.
inline int64_t persistent_bx(int64_t items, int64_t per_wg, int64_t budget, int64_t M) {
    const int64_t bx = (items + per_wg - 1) / per_wg;
    const int64_t cap = budget / M < 1 ? 1 : budget / M;
    return bx > cap ? cap : bx;
}

// The same with the cap rounded up, ceil(budget / M): the whole-flow kernels, one LDS-limited workgroup per CU.  A
// different formula (the two caps differ wherever M does not divide the budget): they stay two functions.
inline int64_t persistent_bx_ceil(int64_t items, int64_t per_wg, int64_t budget, int64_t M) {
    const int64_t bx = (items + per_wg - 1) / per_wg;
    const int64_t cap = (budget + M - 1) / M;
    return bx > cap ? cap : bx;
}

}  // namespace tnf
