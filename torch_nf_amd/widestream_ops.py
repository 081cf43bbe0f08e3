"""Tensor-level wrappers of include/tnf_widestream.h, in the staging vocabulary of _staging.py: a coupling flow with
17 <= num_units <= 64 at any 2 <= D <= 64 and any number of stages, the whole flow in one launch with one or two layers'
operand images streamed through LDS (csrc/flow_wide_stream.hip).

`wide_flow_stream_log_prob_raw` and `wide_flow_stream_forward_raw` are the entries NormFlow routes to (family
`wide_flow_streamed`, behind the switch `NormFlow.wide_flow_streamed`); they take and return what wideflow_ops'
entries do, and accept every shape `wide_flow_stream_supported` covers -- the resident kernel's shapes included.
No autograd: calls that need gradients keep their routes."""
from . import _flow_family
from ._lib import lib, check

COUNT_LOG_PROB, COUNT_FORWARD = 0, 1  # TNF_WIDESTREAM_COUNT_*
SHIPPED_TILES = (1, 2, 4)


def wide_flow_stream_supported(D, S, L, U):
    """tnf_wide_flow_stream_supported: 2 <= D <= 64, 1 <= S <= 1024, 1 <= L <= 5, 17 <= U <= 64 and ONE layer's operand
    image with its fold constants within 150 KB of LDS."""
    return lib.tnf_wide_flow_stream_supported(D, S, L, U) == 1


def lds_bytes(D, L, U):
    """tnf_wide_flow_stream_lds_bytes: the dynamic LDS of a launch (two layers if they fit, else one; 0: no such kernel)."""
    return lib.tnf_wide_flow_stream_lds_bytes(D, L, U)


def tiles(D, S, L, U, M, N):
    """tnf_wide_flow_stream_tiles: the 16-sample tiles per wave that the rule picks for M parameter rows of N samples
    (-1: no such kernel)."""
    return lib.tnf_wide_flow_stream_tiles(D, S, L, U, M, N)


def set_tiles(T):
    """tnf_wide_flow_stream_set_tiles: force T tiles per wave (1, 2 or 4; clamped to the largest the tile shape has) for
    every later launch of the process, or 0: the rule.  Returns the previous setting."""
    return check(lib.tnf_wide_flow_stream_set_tiles(T))


def launch_counts():
    """(log_prob calls, forward calls) that reached their launch."""
    return lib.tnf_wide_flow_stream_launch_count(COUNT_LOG_PROB), lib.tnf_wide_flow_stream_launch_count(COUNT_FORWARD)


def wide_flow_stream_log_prob_raw(z, params, bn_mean, bn_alpha, D, S, L, U, want_lp=True, want_z0=False, want_sld=False):
    """tnf_wide_flow_stream_log_prob_f32: z (M_z, N, D), params (M_p, >= D_params), M_z and M_p in {1, M}
    -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    return _flow_family.log_prob_raw("tnf_wide_flow_stream_log_prob_f32", z, params, bn_mean, bn_alpha, D, S, L, U, want_lp,
                                     want_z0, want_sld)


def wide_flow_stream_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_wide_flow_stream_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M or 1, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.forward_raw("tnf_wide_flow_stream_forward_f32", omega, params, bn_mean, bn_alpha, D, S, L, U,
                                    shared_params=True)
