// The lane-level vocabulary of the device code (gfx950, wave64): vector typedefs, MFMA wrappers, the split-f16
// operand split, wave / row reductions, the power-of-two normalisation, the accumulator-tile transpose and the
// hardware-transcendental forms of exp / log / tanh.  One definition each; what a kernel family builds on top
// (tiles, images, layer bodies) lives in its own header.  Everything here is __forceinline__ and stateless.
#pragma once
#include <hip/hip_runtime.h>

// Timing experiments only; no default build defines them.  TNF_ABLATE == 1 (no transcendental work in sig2) reaches
// every kernel through sig2, as it always did.  The two "no remainder" experiments belong to the whole-flow
// kernels alone: f16_tile.h (TNF_ABLATE == 2) and f16_tile2.h (TNF2_ABL == 4) switch them on before they include
// this header, nothing else does, so the conditional kernels split exactly whatever -D is given.
#ifndef TNF_ABLATE
#define TNF_ABLATE 0
#endif
#ifndef TNF_SPLIT_RTZ_NO_REMAINDER
#define TNF_SPLIT_RTZ_NO_REMAINDER 0
#endif
#ifndef TNF_SPLIT_RNE_NO_REMAINDER
#define TNF_SPLIT_RNE_NO_REMAINDER 0
#endif

namespace tnf {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;  // destination of __builtin_amdgcn_global_load_lds

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kTwoLog2e = 2.88539008177792681472f;
constexpr float kLn2 = 0.69314718055994530942f;

// ---- matrix instructions -------------------------------------------------------------------------------------------
__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f4 mfma16h(h4 a, h4 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f4 mfma32h(h8 a, h8 b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// ---- split-f16 operands --------------------------------------------------------------------------------------------
// v = hi + lo with hi = f16(v), lo = f16(v - hi); an fp32-accurate contraction is three f16 MFMAs (hi.hi + lo.hi +
// hi.lo) with fp32 accumulate.  Two floats -> packed (hi, hi) and (lo, lo) f16 pairs, one dword each.
//
// Inline-asm rule of this code base (measured the hard way, flow_fused2.hip round 2): hipcc neither sees the registers
// an asm VALU instruction READS as results of an in-flight MFMA, nor pads the WAR / WAW hazards of the registers it
// WRITES against MFMAs still reading (SrcC, up to 7 wait states for an 8-pass MFMA) or writing them.  A fresh "=v"
// output may land in exactly such a register -- results then change with the schedule and from run to run.  So an asm
// VALU instruction here only ever (a) reads results of ordinary VALU instructions and (b) writes IN PLACE ("+v") over a
// value an ordinary VALU instruction produced after the MFMAs in question: the compiler resolved every MFMA hazard of
// that register when it scheduled the producer, and it copies the value first (v_mov, visible) if it is still live.
struct HiLo {
    unsigned hi, lo;
};
// v0, v1 <- v - (float)hi as ONE mixed-precision FMA reading the f16 half directly (hipcc does not select
// v_fma_mix_f32 for this pattern; it emits v_cvt_f32_f16 + v_sub_f32).  Exact: the difference of v and its f16
// rounding is representable in fp32.  In place ("+v"): the rule above.
__device__ __forceinline__ void split_remainder(float& v0, float& v1, unsigned hb) {
    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(v0) : "v"(hb));
    asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(v1) : "v"(hb));
}

// round toward zero (v_cvt_pkrtz_f16_f32): the halves never overflow to inf
__device__ __forceinline__ HiLo split2v(float v0, float v1) {
    const unsigned hb = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(v0, v1));
#if TNF_SPLIT_RTZ_NO_REMAINDER
    return HiLo{hb, hb};
#endif
    split_remainder(v0, v1, hb);
    return HiLo{hb, __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(v0, v1))};
}
// round to nearest (v_cvt_pk_f16_f32): |v| >= 65520 gives hi = +-inf, lo = -+inf -- out-of-range inputs are detectable
__device__ __forceinline__ HiLo split2r(float v0, float v1) {
    const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(f2{v0, v1}, h2));
#if TNF_SPLIT_RNE_NO_REMAINDER
    return HiLo{hb, hb};
#endif
    split_remainder(v0, v1, hb);
    return HiLo{hb, __builtin_bit_cast(unsigned, __builtin_convertvector(f2{v0, v1}, h2))};
}
// The same split of v0, v1 with the remainders written over d0, d1 instead: two DEAD values that an ordinary VALU
// instruction produced after the MFMAs (clause (b) of the rule; v0, v1 are ordinary VALU results, clause (a)), so a v
// that stays live is not copied first.  The instructions and their inputs are split2r's: the same bits.
__device__ __forceinline__ HiLo split2r_into(float v0, float v1, float& d0, float& d1) {
    const unsigned hb = __builtin_bit_cast(unsigned, __builtin_convertvector(f2{v0, v1}, h2));
#if TNF_SPLIT_RNE_NO_REMAINDER
    return HiLo{hb, hb};
#endif
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(d0) : "v"(hb), "v"(v0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(d1) : "v"(hb), "v"(v1));
    return HiLo{hb, __builtin_bit_cast(unsigned, __builtin_convertvector(f2{d0, d1}, h2))};
}
// (vector elements cannot bind to references, hence the macro)
#define split2(V0, V1, HI, LO)                \
    do {                                      \
        const HiLo hl_ = split2v((V0), (V1)); \
        (HI) = hl_.hi;                        \
        (LO) = hl_.lo;                        \
    } while (0)

// four values -> hi(4), lo(4); eight -> hi(8), lo(8)
__device__ __forceinline__ void split4(f4 v, h4& hi, h4& lo) {
    const HiLo a = split2v(v[0], v[1]), b = split2v(v[2], v[3]);
    hi = __builtin_bit_cast(h4, u2{a.hi, b.hi});
    lo = __builtin_bit_cast(h4, u2{a.lo, b.lo});
}
__device__ __forceinline__ void split4r(f4 v, h4& hi, h4& lo) {
    const HiLo a = split2r(v[0], v[1]), b = split2r(v[2], v[3]);
    hi = __builtin_bit_cast(h4, u2{a.hi, b.hi});
    lo = __builtin_bit_cast(h4, u2{a.lo, b.lo});
}
__device__ __forceinline__ void split8(f4 v0, f4 v1, h8& hi, h8& lo) {
    const HiLo a = split2v(v0[0], v0[1]), b = split2v(v0[2], v0[3]);
    const HiLo c = split2v(v1[0], v1[1]), d = split2v(v1[2], v1[3]);
    hi = __builtin_bit_cast(h8, u4{a.hi, b.hi, c.hi, d.hi});
    lo = __builtin_bit_cast(h8, u4{a.lo, b.lo, c.lo, d.lo});
}

// ---- cross-lane reductions -----------------------------------------------------------------------------------------
// The offset orders are part of the contract (float sums are order-sensitive): 32 -> 1 for the full wave, 1 -> 8 for
// the 16 sample lanes of a q-group, 16 then 32 for the four q-lanes of a sample.  Every lane gets the result.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float row16_sum(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}
// sum over the four q-lanes that share a sample / an operand row (lanes r, r+16, r+32, r+48)
template <class T>
__device__ __forceinline__ T reduce_q(T v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// ---- power-of-two normalisation ------------------------------------------------------------------------------------
// A maximum mx > 0 (finite) has an exponent k with mx * 2^k in [1, 2); scaling by pow2i(k) is exact.
__device__ __forceinline__ bool pow2_normable(float mx) { return mx > 0.f && mx < 3.0e38f; }
__device__ __forceinline__ int pow2_exponent(float mx, int lo, int hi) {  // clamped to [lo, hi]; mx normable
    int e;
    (void)__builtin_frexpf(mx, &e);  // mx = m 2^e, m in [0.5, 1)
    const int k = 1 - e;
    return k < lo ? lo : (k > hi ? hi : k);
}
__device__ __forceinline__ float pow2i(int k) { return __builtin_ldexpf(1.f, k); }
// the exponent, 0 for mx = 0 / non-finite
__device__ __forceinline__ int pow2_norm(float mx, int lo, int hi) {
    if (!pow2_normable(mx)) return 0;
    return pow2_exponent(mx, lo, hi);
}
// the scale that brings a gradient maximum into [1, 2) (keeps the f16 halves of the deltas normal) and its inverse
struct Pow2Scale {
    float sc, isc;
};
__device__ __forceinline__ Pow2Scale pow2_scale(float mx) {
    Pow2Scale r{1.f, 1.f};
    if (pow2_normable(mx)) {
        const int k = pow2_exponent(mx, -120, 120);
        r.sc = pow2i(k);
        r.isc = pow2i(-k);
    }
    return r;
}

// ---- accumulator tile -> operand tile ------------------------------------------------------------------------------
// 16x16 transpose through LDS (scr: 16 rows of stride 17, bank-conflict-free both ways).  acc layout (lane (s, q),
// reg j = row 4q + j, col s)  ->  operand layout with K = samples (lane (c = lane & 15, kq = lane >> 4),
// reg i = element [row c][sample 4i + kq]).
__device__ __forceinline__ f4 transpose_tile(f4 v, float* scr, int lane) {
    const int s = lane & 15, q = lane >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) scr[(4 * q + j) * 17 + s] = v[j];
    f4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = scr[s * 17 + 4 * i + q];
    return o;
}

// ---- fast transcendentals ------------------------------------------------------------------------------------------
// r = 1/(2^a + 1)  (a = 2 log2(e) x  ->  tanh(x) = 1 - 2r).  2^a -> inf gives r = 0, -> 0 gives r = 1.
__device__ __forceinline__ float sig2(float a) {
#if TNF_ABLATE == 1
    return a;  // timing experiment only: no transcendental work
#else
    return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(a) + 1.0f);
#endif
}
// hardware forms (v_exp_f32 / v_rcp_f32 / v_log_f32, ~1 ulp): the precise library versions cost ~50 VALU instructions
// each and, with two waves per SIMD, that is time the matrix pipe idles
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(kLog2e * x); }
__device__ __forceinline__ float fast_log(float x) { return kLn2 * __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float fast_tanh(float x) { return 1.f - 2.f * sig2(kTwoLog2e * x); }
// log(sigmoid(x)) = min(x, 0) - log(1 + exp(-|x|))
__device__ __forceinline__ float fast_logsigmoid(float x) { return fminf(x, 0.f) - fast_log(1.f + fast_exp(-fabsf(x))); }

}  // namespace tnf
