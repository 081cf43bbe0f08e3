"""Tensor-level wrappers of include/tnf_ctxflow.h, in the staging vocabulary of _staging.py: a coupling flow with one
parameter row per context and 1 <= N <= 31 samples per context, the whole flow in one launch at every 2 <= D <= 64.

`ctx_flow_log_prob_raw` and `ctx_flow_forward_raw` are the entries NormFlow routes to (family `context_rows`, behind the
switch `NormFlow.context_rows`); they return what ops.flow_padded_log_prob_raw and ops.flow_padded_forward_raw return.
No autograd: calls that need gradients keep their routes."""
from . import _flow_family
from ._lib import lib

WAVES_PER_WORKGROUP = 4  # contexts per workgroup of the kernel (csrc/flow_ctx.hip CTX_WAVES): the tests' edge cases
COUNT_LOG_PROB, COUNT_FORWARD = 0, 1  # TNF_CTXFLOW_COUNT_*


def ctx_flow_supported(D, S, L, U, N):
    """tnf_ctx_flow_supported: 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and 1 <= N <= 31."""
    return lib.tnf_ctx_flow_supported(D, S, L, U, N) == 1


def launch_counts():
    """(log_prob calls, forward calls) that reached their launch."""
    return lib.tnf_ctx_flow_launch_count(COUNT_LOG_PROB), lib.tnf_ctx_flow_launch_count(COUNT_FORWARD)


def ctx_flow_log_prob_raw(z, params, bn_mean, bn_alpha, D, S, L, U, want_lp=True, want_z0=False, want_sld=False):
    """tnf_ctx_flow_log_prob_f32: z (M_z, N, D) with M_z in {1, M}, params (M, >= D_params) one row per context
    -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    return _flow_family.log_prob_raw("tnf_ctx_flow_log_prob_f32", z, params, bn_mean, bn_alpha, D, S, L, U, want_lp, want_z0,
                                     want_sld)


def ctx_flow_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_ctx_flow_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.forward_raw("tnf_ctx_flow_forward_f32", omega, params, bn_mean, bn_alpha, D, S, L, U,
                                    shared_params=False)
