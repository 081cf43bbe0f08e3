/* Streamed whole-flow RealNVP ("coupling") kernel for hidden widths 17 <= num_units <= 64 at every width 2 <= D <= 64
 * and any number of stages: plain log_prob, inverse_and_log_det, frozen-statistics forward and sample in ONE launch per
 * call.  tnf_wideflow.h does this with the operand images of all 2 S coupling layers resident in LDS, which caps S (at
 * num_layers = 2: S <= 4 for D <= 32 and U <= 32, S <= 2 for D >= 33, S = 1 for U >= 49, nothing for U >= 49 with
 * L >= 3).  Here one workgroup owns one parameter row, keeps a ring of one or two layers in LDS -- operand image plus
 * fold block, built straight from the packed row -- and walks groups of 128 T samples, held in registers, through all
 * 2 S layers, rebuilding the next layer beside (two slots) or after (one slot) the arithmetic of the current one.  No
 * prepared images, no workspace, no second launch, no atomics; z never round-trips through HBM between layers.
 *
 * tnf_wide_flow_stream_supported(D, S, L, U): 1 exactly for 2 <= D <= 64, 1 <= S <= 1024, 1 <= L <= 5, 17 <= U <= 64 and
 *   4 (floats + 64 HT) <= 153,600 bytes of LDS for ONE layer (floats, HT: tnf_wideflow.h); else 0.  The shapes
 *   tnf_wide_flow_supported covers are covered too.
 * tnf_wide_flow_stream_lds_bytes(D, L, U): the dynamic LDS of a launch: two layers if they fit 153,600 bytes, else one;
 *   0 where no S is supported.  (64, ., 2, 64): 134,656 (two of 67,328); (8, ., 5, 64): 150,400 (one);
 *   (64, ., 5, 64): one layer is 167,168: refused.
 * tnf_wide_flow_stream_tiles(D, S, L, U, M, N): T, the 16-sample tiles a wave holds, that the rule picks for M
 *   parameter rows of N samples: the largest T the tile shape has -- 1, 2, 4; at D >= 33 with U >= 49 only 1, 2, and
 *   only 1 there at L >= 4, where the larger ones would spill -- with M ceil(ceil(N / 16) / (8 T)) >= 256 (a group for
 *   every CU) and ceil(N / 16) > 4 T (tiles for the slots it adds), else 1; -1 for an unsupported shape, M < 1 or N < 0.
 * tnf_wide_flow_stream_set_tiles(T): a process-wide override of that choice, for measurements and tests: 1, 2 or 4
 *   forces it for every later launch (a T above the tile shape's largest runs as that largest), 0 returns to the
 *   rule; returns the previous setting; any other value is TNF_EINVAL and changes nothing.  Results do not depend on T.
 * tnf_wide_flow_stream_launch_count(which): successful calls that reached their launch, per entry; a counter space of
 *   its own (TNF_DIAG_FAMILIES and TNF_WIDEFLOW_COUNTERS are closed sets).  No tnf_diag_launch_count family moves.
 *
 * tnf_wide_flow_stream_log_prob_f32 and tnf_wide_flow_stream_forward_f32 take the arguments of
 * tnf_wide_flow_log_prob_f32 and tnf_wide_flow_forward_f32 (tnf_wideflow.h) with the same meaning, outputs, aliasing
 * rules and N == 0 behaviour, and compute the same bits where both apply.
 * Refused before any launch: a NULL input, no output requested, M_z or M_p < 1 or not in {1, M} (sampling: M_z != M),
 * N < 0, pstride < tnf_flow_num_params(D, S, L, U), z0 == z and z_out == omega are TNF_EINVAL; a shape for which
 * tnf_wide_flow_stream_supported is 0 is TNF_EUNSUPPORTED.  N == 0 returns TNF_OK without a launch.
 * Each successful call is exactly one kernel launch; it does not allocate, does not synchronise and honours
 * tnf_set_launch_gate, so it can be captured into a HIP graph.
 * Included by tnf.h; a header of its own for the reason tnf_mog.h gives.  Bound by torch_nf_amd/_lib.py
 * WIDESTREAM_ENTRIES; tests/test_wide_stream_host.py keeps this header, the exports and that table in step.
 * float32 only; no gradients. */
#ifndef TNF_WIDESTREAM_H
#define TNF_WIDESTREAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { TNF_WIDESTREAM_COUNT_LOG_PROB = 0, TNF_WIDESTREAM_COUNT_FORWARD = 1, TNF_WIDESTREAM_COUNTERS = 2 };
int tnf_wide_flow_stream_supported(int32_t D, int32_t S, int32_t L, int32_t U);
int64_t tnf_wide_flow_stream_lds_bytes(int32_t D, int32_t L, int32_t U);
int tnf_wide_flow_stream_tiles(int32_t D, int32_t S, int32_t L, int32_t U, int64_t M, int64_t N);
int tnf_wide_flow_stream_set_tiles(int32_t T);
int64_t tnf_wide_flow_stream_launch_count(int32_t which);
int tnf_wide_flow_stream_log_prob_f32(const float* z, const float* params, const float* bn_mean, const float* bn_alpha,
                                      float* log_prob, float* z0, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N,
                                      int32_t D, int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream);
int tnf_wide_flow_stream_forward_f32(const float* omega, const float* params, const float* bn_mean, const float* bn_alpha,
                                     float* z_out, float* sum_log_det, int64_t M_z, int64_t M_p, int64_t N, int32_t D,
                                     int32_t S, int32_t L, int32_t U, int64_t pstride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TNF_WIDESTREAM_H */
