// The counter-based random stream of the simulators (include/tnf_abc.h, include/tnf_hebb.h): Philox4x32-10 and the
// Box-Muller pair that turns two of its words into two standard normals.  One definition each, shared by abc_kernels.hip
// and hebb_kernels.hip, so that the two families draw the same bits from the same (key, counter).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tnf {

__device__ __forceinline__ void abc_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// one Box-Muller pair; the products are kept as products (no contraction into a consumer's FMA), so the noise entry
// and the in-kernel stream give the same bits
__device__ __forceinline__ void abc_pair(uint32_t wa, uint32_t wb, float& n0, float& n1) {
    const float u1 = ((float)(wa >> 8) + 0.5f) * 0x1p-24f;
    const float u2 = (float)(wb >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.28318530717958647692f * u2, &s, &c);
    n0 = __fmul_rn(r, c);
    n1 = __fmul_rn(r, s);
}

}  // namespace tnf
