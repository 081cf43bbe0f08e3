/* Training a RealNVP ("coupling") flow of any width 2 <= D <= 63 (D != 32) through the one-kernel reversible backward
 * (tnf_flow_log_prob_bwd_rev_f32, which exists at D = 32 and 64 only).  A coupling flow of width D is exactly a flow of
 * width D' = 2H with zeros in the extra slots, H = 16 for D <= 31 and 32 for 33 <= D <= 63 (the rule of the padded
 * forward, tnf_flow_padded_log_prob_f32): zero weight rows and columns give s = t = 0 on the padded outputs, identity
 * BatchNorm statistics and zero Affine rows keep the padded features at 0 through every layer, and the gradients at the
 * real slots are the real gradients.  The entries here move rows and parameter rows into and out of that embedded layout
 * and run the existing backward on it; no existing kernel changes.  Serves autograd through NormFlow.log_prob
 * (density_estimator.py:408-416 of the reference) at the widths the reference demonstrates with coupling flows (D = 4 in
 * notebooks/LFI_gauss.ipynb, D = 2, 4, 5, 8 in its tests).  Included by tnf.h; a header of its own for the reason
 * tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py PADTRAIN_SIGNATURES; tests/test_padded_train_host.py keeps this header,
 * the exports and that table in step.  float32 only.
 *
 * THE EMBEDDED LAYOUT, h = D / 2 (integer division):
 *   features    f -> f for f < h, else H + (f - h): the first half of a row holds features 0 .. h-1, the second half
 *               features h .. D-1 (the split of bijectors.py:155-165 for every layer), each half zero-padded to H.  Used by
 *               the rows (z0, g_z), the BatchNorm statistics (bijectors.py:389-426; mean 0 and alpha 1 at padding) and the
 *               Affine block [alpha | shift] (bijectors.py:277-318; zeros at padding).
 *   parameters  a row is, per stage, [RealNVP(upper) | RealNVP(lower) | Affine (2D)] (density_estimator.py:260-270); a
 *               RealNVP block is [W_t | W_s | b_t | b_s] per MLP layer with W row-major [in][out] (bijectors.py:222-242).
 *               First layer din x U -> H x U: rows >= din are padding.  Hidden layers U x U: unchanged.  Last layer
 *               U x dout -> U x H: columns >= dout, and bias entries >= dout, are padding.  din / dout follow the
 *               reference's h / h+1 rule for odd D and for upper / lower (bijectors.py:163-165, 250-254).
 *   The map from a real parameter index to its embedded index is strictly increasing, so padding is exactly the gaps
 *   between consecutive images.
 *
 * tnf_flow_padded_width(D): 2H = 32 for 2 <= D <= 31, 64 for 33 <= D <= 63, else 0.
 * tnf_flow_padded_train_supported(D, S, L, U): 1 exactly when tnf_flow_padded_supported(D, S, L, U) and
 *   tnf_flow_train_rev_supported(2H, S, L, U), else 0.
 * tnf_flow_padded_embed_index(D, S, L, U, k): host only.  The index in the (2H, S, L, U) row of real parameter index k of
 *   the (D, S, L, U) row (tnf_flow_num_params each); -1 when k is out of range or tnf_flow_padded_width(D) is 0, S < 1,
 *   L < 1 or U < 1.
 * tnf_padtrain_launch_count(which): launches per entry, a counter space of its own (TNF_DIAG_FAMILIES is a closed set).
 *
 * The four kernels (each one launch; plain vector loads and stores, no atomics, no allocation, no synchronisation, so
 * they can be captured into a HIP graph).  Refused before any launch: NULL pointers, negative R / M_p, a row stride
 * shorter than the row and an embedded pointer that is not 16-byte aligned are TNF_EINVAL; a (D, S, L, U) for which
 * tnf_flow_padded_train_supported is 0 -- for the two row kernels a D whose tnf_flow_padded_width is 0 -- is
 * TNF_EUNSUPPORTED.  R == 0 / M_p == 0 return TNF_OK without a launch.
 *   tnf_flow_padded_embed_rows_f32    rows (R, D) at 4-byte alignment -> out (R, 2H); the padding zeros are written by the
 *                                     kernel itself.
 *   tnf_flow_padded_gather_rows_f32   the inverse: rows (R, 2H) -> out (R, D); padding is not read back.
 *   tnf_flow_padded_embed_params_f32  params (M_p, pstride) -> params_out (M_p, P'), P' = tnf_flow_num_params(2H, S, L, U),
 *                                     zeros at padding; and bn_mean / bn_alpha (2S, D) -> (2S, 2H).
 *   tnf_flow_padded_gather_params_f32 g (M_p, P') -> g_out (M_p, gpstride): only the real slots are read (the padded slots
 *                                     of a gradient row hold non-zero sums); g_out beyond the real row is left as it is.
 *
 * tnf_flow_padded_log_prob_bwd_f32: the backward of log_prob from z0 (M, N, D), what tnf_flow_padded_log_prob_f32 keeps.
 *   Embeds z0, the parameter rows and the statistics into the workspace, runs the reversible backward at width 2H
 *   (arguments, overflow flag and bit-reproducibility as tnf_flow_log_prob_bwd_rev_f32) and gathers g_params
 *   (M_p, gpstride; written over the real row) and, unless g_z is NULL, g_z (M, N, D).  M_p is 1 or M.  Checked before any
 *   launch: a NULL z0 / params / bn_mean / bn_alpha / g_log_prob / g_params, M < 1, M_p not in {1, M}, N < 0 and
 *   pstride or gpstride shorter than tnf_flow_num_params(D, S, L, U) are TNF_EINVAL; an unsupported shape is
 *   TNF_EUNSUPPORTED; a NULL or short workspace is TNF_EWORKSPACE.  N == 0 returns TNF_OK without a launch.
 * tnf_flow_padded_train_workspace_bytes: its workspace -- the embedded z0 and g_z, parameter and gradient rows, statistics
 *   and the workspace of the backward at width 2H; TNF_EINVAL / TNF_EUNSUPPORTED as above. */
#ifndef TNF_PADTRAIN_H
#define TNF_PADTRAIN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum {
    TNF_PADTRAIN_COUNT_EMBED_ROWS = 0,
    TNF_PADTRAIN_COUNT_GATHER_ROWS = 1,
    TNF_PADTRAIN_COUNT_EMBED_PARAMS = 2,
    TNF_PADTRAIN_COUNT_GATHER_PARAMS = 3,
    TNF_PADTRAIN_COUNT_BWD = 4,
    TNF_PADTRAIN_COUNTERS = 5
};
int tnf_flow_padded_train_supported(int32_t D, int32_t S, int32_t L, int32_t U);
int tnf_flow_padded_width(int32_t D);
int64_t tnf_flow_padded_embed_index(int32_t D, int32_t S, int32_t L, int32_t U, int64_t k);
int64_t tnf_padtrain_launch_count(int32_t which);
int tnf_flow_padded_embed_rows_f32(const float* rows, float* out, int64_t R, int32_t D, void* stream);
int tnf_flow_padded_gather_rows_f32(const float* rows, float* out, int64_t R, int32_t D, void* stream);
int tnf_flow_padded_embed_params_f32(const float* params, const float* bn_mean, const float* bn_alpha, float* params_out,
                                     float* bn_mean_out, float* bn_alpha_out, int64_t M_p, int32_t D, int32_t S, int32_t L,
                                     int32_t U, int64_t pstride, void* stream);
int tnf_flow_padded_gather_params_f32(const float* g, float* g_out, int64_t M_p, int32_t D, int32_t S, int32_t L, int32_t U,
                                      int64_t gpstride, void* stream);
int64_t tnf_flow_padded_train_workspace_bytes(int64_t M, int64_t M_p, int64_t N, int32_t D, int32_t S, int32_t L, int32_t U);
int tnf_flow_padded_log_prob_bwd_f32(const float* z0, const float* params, const float* bn_mean, const float* bn_alpha,
                                     const float* g_log_prob, float* g_z, float* g_params, int64_t M, int64_t M_p, int64_t N,
                                     int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, int64_t gpstride,
                                     void* workspace, int64_t workspace_bytes, int32_t* overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_PADTRAIN_H */
