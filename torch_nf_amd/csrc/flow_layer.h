// Host only: "coupling layer c of a flow", for the per-layer chains that launch one kernel per layer.
#pragma once
#include "tnf_common.h"

namespace tnf {

// Layer c = 0 .. 2S-1 in sampling order: stage c / 2, its upper transform (even c) or its lower one (odd c).
struct FlowLayerAt {
    int64_t poff;          // the layer's parameters inside a parameter row (and its gradient inside a gradient row)
    const float* image;    // its prepared operand image in an (Mp, 2S, img_floats) array ...
    int64_t image_stride;  // ... and the floats between two parameter rows there
    int64_t fold_off;      // its [A (D) | B (D)] constants in an (Mp, 2S, 2, D) fold array ...
    int64_t fold_stride;   // ... and the floats between two parameter rows there
    int upper;
};

inline FlowLayerAt flow_layer_at(const FlowLayout& fl, int c, int S, int D, const float* images, int64_t img_floats) {
    FlowLayerAt at;
    at.poff = (c >> 1) * fl.stage + ((c & 1) ? fl.p_up : 0);
    at.image = images + (int64_t)c * img_floats;
    at.image_stride = (int64_t)(2 * S) * img_floats;
    at.fold_off = (int64_t)c * 2 * D;
    at.fold_stride = (int64_t)(2 * S) * 2 * D;
    at.upper = (c & 1) ? 0 : 1;
    return at;
}

// The fields MfmaLayerArgs and BwdArgs share.  The folds stay with the caller: which of pre / post / fold / g_fold they
// feed, and from which array, differs between the chains.
template <class Args>
inline void set_flow_layer(Args& a, const FlowLayerAt& at, const float* params, int64_t pstride, int U) {
    a.params = params + at.poff;
    a.pstride = pstride;
    a.image = at.image;
    a.image_stride = at.image_stride;
    a.U = U;
    a.upper = at.upper;
}

}  // namespace tnf
