// Split-f16 operand image of one coupling layer, shared by the whole-flow kernels (flow_fused_f16.hip,
// flow_bwd_f16.hip).  The split itself (round toward zero here) is wave_prims.h's; see flow_fused_f16.hip for the
// measurements.
#pragma once
#if defined(TNF_ABLATE) && TNF_ABLATE == 2  // timing experiment only: split without remainder (scope: wave_prims.h)
#define TNF_SPLIT_RTZ_NO_REMAINDER 1
#endif
#include "mfma_tile.h"

namespace tnf {

// LDS / global image of one layer's split-f16 operands: 16-byte groups [g][lane], then the
// fp32 bias groups [g][q][4] exactly as in LdsLayerImage.
template <int H, int L>
struct F16Image {
    static constexpr int HT = (H + 15) / 16;
    static constexpr int NW0 = (H == 32) ? 4 : 2;            // layer-0 groups
    static constexpr int NWG = NW0 + 2 * (L - 1) + 2 * HT;   // 16-byte-per-lane groups
    static constexpr int NBG = 2 + 2 * (L - 1) + 2 * HT;
    static constexpr int FLOATS = NWG * 256 + NBG * 16;      // size in 4-byte units
    __device__ static constexpr int g_w0(int net, int part) { return (H == 32) ? net * 2 + part : net; }
    __device__ static constexpr int g_wh(int l, int net) { return NW0 + 2 * l + net; }
    __device__ static constexpr int g_w2(int net, int mo) { return NW0 + 2 * (L - 1) + net * HT + mo; }
    __device__ static constexpr int b_b0(int net) { return net; }
    __device__ static constexpr int b_bh(int l, int net) { return 2 + 2 * l + net; }
    __device__ static constexpr int b_b2(int net, int mo) { return 2 + 2 * (L - 1) + net * HT + mo; }
};

static_assert(F16Image<32, 3>::FLOATS <= LdsLayerImage<32, 3>::FLOATS, "f16 image must fit the fp32 image slot");
static_assert(F16Image<16, 3>::FLOATS <= LdsLayerImage<16, 3>::FLOATS, "f16 image must fit the fp32 image slot");

// ---------------------------------------------------------------------------
// Prep: one wave per (layer, context) folds + gathers the fp32 operands (load_layer_w),
// splits them and writes the f16 image.
// ---------------------------------------------------------------------------
// one wave: gather + fold + split the operands of the coupling layer whose parameters start at `p` and
// write its image to `img` (global memory in the prep kernel, LDS when the flow kernel builds its own)
template <int H, int L>
__device__ __forceinline__ void build_f16_image(float* img, const float* __restrict__ p, int U, int lane) {
    typedef F16Image<H, L> Img;
    constexpr int HT = Img::HT;
    LayerW<H, L> w;
    load_layer_w<H, L>(w, p, U, lane);
    u4* grp = reinterpret_cast<u4*>(img) + lane;  // group g at grp[g * 64]
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        if constexpr (H == 32) {
            u4 hi, lo;
#pragma unroll
            for (int p = 0; p < 4; ++p) split2(w.w0[net][2 * p], w.w0[net][2 * p + 1], hi[p], lo[p]);
            grp[Img::g_w0(net, 0) * 64] = hi;
            grp[Img::g_w0(net, 1) * 64] = lo;
        } else {
            u4 v;
            split2(w.w0[net][0], w.w0[net][1], v[0], v[2]);
            split2(w.w0[net][2], w.w0[net][3], v[1], v[3]);
            grp[Img::g_w0(net, 0) * 64] = v;  // [hi(4) | lo(4)]
        }
#pragma unroll
        for (int l = 0; l < L - 1; ++l) {
            u4 v;
            split2(w.wh[l][net][0], w.wh[l][net][1], v[0], v[2]);
            split2(w.wh[l][net][2], w.wh[l][net][3], v[1], v[3]);
            grp[Img::g_wh(l, net) * 64] = v;
        }
#pragma unroll
        for (int mo = 0; mo < HT; ++mo) {
            u4 v;
            split2(w.w2[net][mo][0], w.w2[net][mo][1], v[0], v[2]);
            split2(w.w2[net][mo][2], w.w2[net][mo][3], v[1], v[3]);
            grp[Img::g_w2(net, mo) * 64] = v;
        }
    }
    if ((lane & 15) == 0) {
        float* bl = img + Img::NWG * 256 + (lane >> 4) * 4;
#pragma unroll
        for (int net = 0; net < 2; ++net) {
            *reinterpret_cast<f4*>(bl + Img::b_b0(net) * 16) = w.b0[net];
#pragma unroll
            for (int l = 0; l < L - 1; ++l) *reinterpret_cast<f4*>(bl + Img::b_bh(l, net) * 16) = w.bh[l][net];
#pragma unroll
            for (int mo = 0; mo < HT; ++mo) *reinterpret_cast<f4*>(bl + Img::b_b2(net, mo) * 16) = w.b2[net][mo];
        }
    }
}

}  // namespace tnf
