// Stand-alone check of torch_nf_amd/csrc/dispatch.h (no HIP): every dispatcher hands its lambda the compile-time value
// the launchers' hand-written ladders chose for the same run-time value, and returns what the lambda returns;
// persistent_bx / persistent_bx_ceil equal the literal clamps they replace.  Built and run by test_dispatch_host.py.
#include <stdio.h>

#include <initializer_list>
#include <type_traits>

#include "../torch_nf_amd/csrc/dispatch.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

using namespace tnf;

int main() {
    // dispatch_hl: D == 64 -> H = 32, anything else -> 16;  L == 1, L == 2, anything else -> 3
    for (int D : {32, 64})
        for (int L : {1, 2, 3}) {
            const int got = dispatch_hl(D, L, [](auto h, auto l) {
                static_assert(std::is_same<typename decltype(h)::value_type, int>::value, "H is an int constant");
                constexpr int H = decltype(h)::value, LL = decltype(l)::value;  // usable as template arguments
                return 100 * H + LL;
            });
            CHECK(got == 100 * (D == 64 ? 32 : 16) + L);
        }
    CHECK(dispatch_hl(48, 7, [](auto h, auto l) { return 100 * h() + l(); }) == 1603);  // the ladders' else arms

    // dispatch_1to4: 1, 2, 3, and everything else is 4 (the switches' default:)
    for (int n : {0, 1, 2, 3, 4, 5}) {
        const int got = dispatch_1to4(n, [](auto t) {
            constexpr int T = decltype(t)::value;
            return T;
        });
        CHECK(got == (n >= 1 && n <= 3 ? n : 4));
    }

    // dispatch_bool: ints as the launchers pass them (inverse, forward) and bools
    for (int flag : {0, 1, 2}) {
        const int got = dispatch_bool(flag, [](auto b) {
            constexpr bool B = decltype(b)::value;
            return B ? 7 : 3;
        });
        CHECK(got == (flag ? 7 : 3));
    }

    // dispatch_dtype: TNF_F32 -> float, TNF_F64 -> double; the lambda's own return type comes back
    CHECK(dispatch_dtype(TNF_F32, [](auto t) { return sizeof(t); }) == 4);
    CHECK(dispatch_dtype(TNF_F64, [](auto t) { return sizeof(t); }) == 8);
    CHECK(dispatch_dtype(TNF_F32, [](auto t) { return std::is_same<decltype(t), float>::value; }));
    CHECK(dispatch_dtype(TNF_F64, [](auto t) { return std::is_same<decltype(t), double>::value; }));

    // nesting: three levels in one expression, each value reaching the innermost lambda
    for (int ht : {1, 4})
        for (int ut : {2, 3})
            for (int inv : {0, 1}) {
                const long got = dispatch_1to4(ht, [&](auto a) {
                    return dispatch_1to4(ut, [&](auto b) {
                        return dispatch_bool(inv, [&](auto c) { return 100L * a() + 10L * b() + (c() ? 1 : 0); });
                    });
                });
                CHECK(got == 100L * ht + 10L * ut + inv);
            }
    int calls = 0;  // void lambdas (launchers that cannot fail) dispatch too, exactly once
    dispatch_hl(64, 2, [&](auto, auto) { ++calls; });
    CHECK(calls == 1);

    // the persistent-grid clamps against the literal code they replace
    const int64_t items_v[] = {0, 1, 3, 4, 5, 1000000};
    // budgets in use: 512 (coupling_bwd_mfma, wide backward), 1024 (coupling_wide, maf_kernels), 2048 (maf_mfma, coupling_mfma)
    for (int64_t budget : {512, 1024, 2048})
        for (int64_t items : items_v)
            for (int64_t M : {(int64_t)1, (int64_t)2, budget, budget + 1, (int64_t)1000000})
                for (int64_t per_wg : {1, 4}) {
                    int64_t bx = (items + per_wg - 1) / per_wg;
                    int64_t cap = budget / M;
                    if (cap < 1) cap = 1;
                    if (bx > cap) bx = cap;
                    CHECK(persistent_bx(items, per_wg, budget, M) == bx);
                }
    for (int64_t budget : {256})  // the whole-flow kernels (256 * TNF2_RANGE_WGPC with its default of 1)
        for (int64_t items : items_v)
            for (int64_t M : {(int64_t)1, (int64_t)2, budget, budget + 1, (int64_t)1000000})
                for (int64_t per_wg : {8, 12}) {
                    int64_t bx = (items + per_wg - 1) / per_wg;
                    int64_t cap = (budget + M - 1) / M;
                    if (bx > cap) bx = cap;
                    CHECK(persistent_bx_ceil(items, per_wg, budget, M) == bx);
                }
    CHECK(persistent_bx(1000000, 4, 512, 3) == 170 && persistent_bx_ceil(1000000, 4, 512, 3) == 171);  // two formulas

    if (failures) return 1;
    printf("dispatch_host: ok\n");
    return 0;
}
