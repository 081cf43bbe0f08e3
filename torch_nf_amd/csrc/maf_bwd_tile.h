// What the two matrix-pipe MAF backward kernels share: maf_bwd_mfma_kernel (maf_bwd_mfma.hip, the backward of the inverse
// direction) and maf_sample_bwd_kernel (maf_sample_bwd.hip, the backward of the sampling direction).  One group numbering
// for the folded image, the transposed image and the weight-gradient accumulators; the image build; the LDS sizing; the
// grid of the tile walk; the masked flush of plain-float accumulators.
#pragma once
#include "mfma_tile.h"
#include "launch.h"

namespace tnf {

struct MafBLayout {  // group numbering shared by the folded image, the transposed image and the accumulators
    int UT, DT, L;
    __host__ __device__ int n0() const { return 2 * UT * DT; }
    __host__ __device__ int nh() const { return 2 * UT * UT; }
    __host__ __device__ int NWG() const { return n0() + (L - 1) * nh() + n0(); }
    __host__ __device__ int NBG() const { return (L - 1) * 2 * UT + 2 * DT; }
    // (net, out tile, in tile) of each layer
    __host__ __device__ int g0(int net, int ut, int mm) const { return (net * UT + ut) * DT + mm; }
    __host__ __device__ int gh(int l, int net, int uo, int ui) const { return n0() + l * nh() + (net * UT + uo) * UT + ui; }
    __host__ __device__ int g2(int net, int mo, int ui) const { return n0() + (L - 1) * nh() + (net * DT + mo) * UT + ui; }
    __host__ __device__ int bh(int l, int net, int uo) const { return l * 2 * UT + net * UT + uo; }
    __host__ __device__ int b2(int net, int mo) const { return (L - 1) * 2 * UT + net * DT + mo; }
    __host__ __device__ int fwd_floats() const { return NWG() * 256 + NBG() * 16; }
};

// folded forward image (same maths as build_maf_image of maf_mfma.hip) and the plain transposed image:
// group (net, out tile, in tile), lane (r, q): W*M [in = 16 it + r][out = 16 ot + 4q + j].
// The (layer, net, out tile) units are dealt round-robin to the workgroup's `nwaves` waves: with one
// workgroup per context the build is on the critical path of every context.
__device__ void build_maf_bwd_images(float* fimg, float* timg, const float* __restrict__ p0, const float* __restrict__ mk0,
                                     MafBLayout wl, int D, int U, int lane, int wave, int nwaves, int bf) {
    const int r = lane & 15, q = lane >> 4;
    float* fw = fimg + lane * 4;
    float* fb = fimg + wl.NWG() * 256 + q * 4;
    float* tw = timg + lane * 4;
    const bool bias_lane = r == 0;
    int unit = 0;
    const float* p = p0;
    const float* mk = mk0;
    for (int layer = 0; layer <= wl.L; ++layer) {
        const int din = layer == 0 ? D : U, dout = layer == wl.L ? D : U;
        const int IT = layer == 0 ? wl.DT : wl.UT, OT = layer == wl.L ? wl.DT : wl.UT;
        const float* w[2] = {p, p + din * dout};
        for (int net = 0; net < 2; ++net) {
            // scale of the folded weights: layer 0 feeds a tanh (c = 2 log2 e); later layers consume
            // r = (1 - tanh)/2 (factor -2) and feed a tanh (c) or the outputs (1 for mu, log2 e for alpha)
            const float outsc = layer == wl.L ? (net == 0 ? 1.f : kLog2e) : kTwoLog2e;
            const float wsc = layer == 0 ? outsc : -2.f * outsc;
            for (int ot = 0; ot < OT; ++ot, ++unit) {
                if (unit % nwaves != wave) continue;
                const int g_base = layer == 0 ? wl.g0(net, ot, 0) : (layer == wl.L ? wl.g2(net, ot, 0) : wl.gh(layer - 1, net, ot, 0));
                float csum = 0.f;
                for (int it = 0; it < IT; ++it) {
                    f4 vf, vt;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // folded: row = output unit 16 ot + r, K = input 16 it + 4q + j
                        const int o = 16 * ot + r, k = 16 * it + 4 * q + j;
                        const bool ok = k < din && o < dout;
                        const float raw = ld_sel(w[net], k * dout + o, ok) * ld_sel(mk, k * dout + o, ok);
                        csum += raw;
                        vf[j] = wsc * raw;
                        // transposed: row = input 16 it + r, K = output 16 ot + 4q + j
                        const int k2 = 16 * it + r, o2 = 16 * ot + 4 * q + j;
                        const bool ok2 = k2 < din && o2 < dout;
                        vt[j] = ld_sel(w[net], k2 * dout + o2, ok2) * ld_sel(mk, k2 * dout + o2, ok2);
                    }
                    *reinterpret_cast<f4*>(fw + (g_base + it) * 256) = rbf16_4(vf, bf);
                    *reinterpret_cast<f4*>(tw + (g_base + it) * 256) = rbf16_4(vt, bf);
                }
                if (layer > 0) {  // accumulator initial values: column sums (there are no biases in MAF)
                    csum = reduce_q(csum);
                    f4 bv;
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = outsc * __shfl(csum, 4 * q + j);
                    const int bg = layer == wl.L ? wl.b2(net, ot) : wl.bh(layer - 1, net, ot);
                    if (bias_lane) *reinterpret_cast<f4*>(fb + bg * 16) = bv;
                }
            }
        }
        p += 2 * din * dout;
        mk += din * dout;
    }
}

constexpr int kMafLMax = 3;

// ---- flush: tile (out tile ot, in tile it) element (o = 16 ot + 4q + j, k = 16 it + (lane & 15)) ----
// The `nacc` accumulator copies leave LDS once, masked: plain stores when the workgroup owns the gradient row (`own`),
// otherwise one atomic per non-zero parameter per workgroup.  NEG: the negated sum is what leaves.  (maf_bwd_mfma_kernel
// keeps its own copy of this loop, with the fixed-point decode in it: calling this one changed its machine code.)
template <int DT, int UT, bool NEG>
__device__ __forceinline__ void maf_bwd_flush(const float* gacc, int nacc, MafBLayout wl, float* gp, const float* mk, int D,
                                              int U, bool own, int lane, int wave) {
    const int s = lane & 15, q = lane >> 4;
    const int L = wl.L, NWG = wl.NWG();
    int64_t off = 0, moff = 0;
    for (int layer = 0; layer <= L; ++layer) {
        const int din = layer == 0 ? D : U, dout = layer == L ? D : U;
        const int IT = layer == 0 ? DT : UT, OT = layer == L ? DT : UT;
        const int64_t nw = (int64_t)din * dout;
        for (int t = wave; t < 2 * OT * IT; t += 4) {
            const int net = t / (OT * IT), rem = t - net * OT * IT, ot = rem / IT, it = rem - ot * IT;
            const int gidx = layer == 0 ? wl.g0(net, ot, it) : (layer == L ? wl.g2(net, ot, it) : wl.gh(layer - 1, net, ot, it));
            f4 v = *reinterpret_cast<const f4*>(gacc + (gidx * 64 + lane) * 4);
            for (int c = 1; c < nacc; ++c) v += *reinterpret_cast<const f4*>(gacc + c * NWG * 256 + (gidx * 64 + lane) * 4);
            if (NEG) v = -v;
            const int k = 16 * it + s;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = 16 * ot + 4 * q + j;
                if (k < din && o < dout) {
                    const int64_t idx = (int64_t)k * dout + o;
                    const float val = v[j] * mk[moff + idx];
                    float* dst = gp + off + net * nw + idx;
                    if (own) *dst = val;
                    else if (val != 0.f) atomicAdd(dst, val);
                }
            }
        }
        off += 2 * nw;
        moff += nw;
    }
}

inline MafBLayout maf_blayout(int D, int L, int U) {
    MafBLayout wl;
    wl.UT = (U + 15) / 16;
    wl.DT = (D + 15) / 16;
    wl.L = L;
    return wl;
}

// images | (1 + nacc) x the weight groups (transposed image, accumulator copies) | per-wave transpose scratch | constants
inline size_t maf_bwd_smem(const MafBLayout& wl, int nacc = 1) {
    return (size_t)(wl.fwd_floats() + (1 + nacc) * wl.NWG() * 256 + 4 * 2 * 272 + 11 * 16 * wl.DT + 4) * sizeof(float);
}

// one private accumulator copy per wave where four fit the LDS, else one shared copy
inline int maf_bwd_nacc(int D, int L, int U) { return maf_bwd_smem(maf_blayout(D, L, U), 4) <= 156 * 1024 ? 4 : 1; }

// the tile walk: 4 waves x 16-sample tiles, grid-stride.  A workgroup per context owns that context's gradient row
// (plain stores); one shared row is walked by a persistent grid of at most 512 workgroups.
inline dim3 maf_bwd_grid(int64_t M, int64_t Mp, int64_t N) {
    const int64_t ntiles = (N + 15) / 16;
    int64_t bx = (ntiles + 3) / 4;
    if (Mp > 1) bx = 1;
    else if (bx > 512) bx = 512;
    return grid_xm(bx, M);
}

}  // namespace tnf
