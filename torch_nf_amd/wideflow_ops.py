"""Tensor-level wrappers of include/tnf_wideflow.h, in the staging vocabulary of _staging.py: a coupling flow with
17 <= num_units <= 64 at any 2 <= D <= 64, the whole flow in one launch.

`wide_flow_log_prob_raw` and `wide_flow_forward_raw` are the entries NormFlow routes to (family `wide_flow`, behind the
switch `NormFlow.wide_flow`); they return what ops.flow_padded_log_prob_raw and ctxflow_ops.ctx_flow_forward_raw return.
No autograd: calls that need gradients keep their routes."""
from . import _flow_family
from ._lib import lib

COUNT_LOG_PROB, COUNT_FORWARD = 0, 1  # TNF_WIDEFLOW_COUNT_*


def wide_flow_supported(D, S, L, U):
    """tnf_wide_flow_supported: 2 <= D <= 64, S >= 1, 1 <= L <= 5, 17 <= U <= 64 and the 2 S operand images with their
    fold constants within 150 KB of LDS."""
    return lib.tnf_wide_flow_supported(D, S, L, U) == 1


def launch_counts():
    """(log_prob calls, forward calls) that reached their launch."""
    return lib.tnf_wide_flow_launch_count(COUNT_LOG_PROB), lib.tnf_wide_flow_launch_count(COUNT_FORWARD)


def wide_flow_log_prob_raw(z, params, bn_mean, bn_alpha, D, S, L, U, want_lp=True, want_z0=False, want_sld=False):
    """tnf_wide_flow_log_prob_f32: z (M_z, N, D), params (M_p, >= D_params), M_z and M_p in {1, M}
    -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    return _flow_family.log_prob_raw("tnf_wide_flow_log_prob_f32", z, params, bn_mean, bn_alpha, D, S, L, U, want_lp,
                                     want_z0, want_sld)


def wide_flow_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_wide_flow_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M or 1, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.forward_raw("tnf_wide_flow_forward_f32", omega, params, bn_mean, bn_alpha, D, S, L, U,
                                    shared_params=True)
