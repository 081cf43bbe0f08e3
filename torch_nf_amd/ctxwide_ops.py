"""Tensor-level wrappers of include/tnf_ctxwide.h, in the staging vocabulary of _staging.py: a coupling flow with
17 <= num_units <= 64, one parameter row per context and 1 <= N <= 31 samples per context -- the whole flow in one launch
(one workgroup per context, one layer's operand image resident at a time), and log_prob under autograd as one launch each
way (the forward keeps z0; the backward is reversible), at every 2 <= D <= 64.

`ctx_wide_log_prob_raw` and `ctx_wide_forward_raw` are the entries NormFlow routes to behind the switch
`NormFlow.wide_context_rows` (family `context_rows_wide`); they return what ctxflow_ops.ctx_flow_log_prob_raw and
ctx_flow_forward_raw return.  `ctx_wide_log_prob_train` is the autograd entry behind `NormFlow.wide_context_training`
(family `train_context_wide`).  The backward kernel alone has the `_raw` wrapper, used by tools/ctxwidebench.py and the
tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
from . import _flow_family
from ._lib import lib

COUNT_LOG_PROB, COUNT_FORWARD, COUNT_LOG_PROB_BWD = 0, 1, 2  # TNF_CTXWIDE_COUNT_*
LDS_FORWARD, LDS_BACKWARD = 0, 1  # `which` of tnf_ctx_wide_lds_bytes


def ctx_wide_supported(D, S, L, U, N):
    """tnf_ctx_wide_supported: 2 <= D <= 64, S >= 1, 1 <= L <= 5, 17 <= U <= 64, 1 <= N <= 31 and one layer's operand
    image within 150 KB of LDS (all but L = 5 at D >= 33 with U >= 49)."""
    return lib.tnf_ctx_wide_supported(D, S, L, U, N) == 1


def ctx_wide_train_supported(D, S, L, U, N):
    """tnf_ctx_wide_train_supported: the same domain with 1 <= L <= 3 and the context's backward slice within 150 KB of
    LDS (all of L <= 2, all of L = 3 up to 48 units)."""
    return lib.tnf_ctx_wide_train_supported(D, S, L, U, N) == 1


def lds_bytes(which, D, S, L, U, N):
    """tnf_ctx_wide_lds_bytes: the dynamic LDS of the forward (LDS_FORWARD) or backward (LDS_BACKWARD) launch, or -1."""
    return lib.tnf_ctx_wide_lds_bytes(which, D, S, L, U, N)


def launch_counts():
    """(log_prob calls, forward calls, backward calls) that reached their launch."""
    return tuple(lib.tnf_ctx_wide_launch_count(i) for i in (COUNT_LOG_PROB, COUNT_FORWARD, COUNT_LOG_PROB_BWD))


def ctx_wide_log_prob_raw(z, params, bn_mean, bn_alpha, D, S, L, U, want_lp=True, want_z0=False, want_sld=False):
    """tnf_ctx_wide_log_prob_f32: z (M_z, N, D) with M_z in {1, M}, params (M, >= D_params) one row per context
    -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    return _flow_family.log_prob_raw("tnf_ctx_wide_log_prob_f32", z, params, bn_mean, bn_alpha, D, S, L, U, want_lp, want_z0,
                                     want_sld)


def ctx_wide_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_ctx_wide_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.forward_raw("tnf_ctx_wide_forward_f32", omega, params, bn_mean, bn_alpha, D, S, L, U,
                                    shared_params=False)


def ctx_wide_log_prob_bwd_raw(z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U, want_gz=True):
    """tnf_ctx_wide_log_prob_bwd_f32: z0 (M, N, D) as the forward kept it, params (M, >= D_params) one row per context,
    g_lp (M, N) -> (g_params in params' shape, trailing columns zero; g_z (M, N, D) | None), one launch."""
    return _flow_family.log_prob_bwd_raw("tnf_ctx_wide_log_prob_bwd_f32", z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U,
                                         want_gz)


def ctx_wide_log_prob_train(z, params, bn_mean, bn_alpha, D, S, L, U):
    """log_prob (M, N) with autograd through the wide per-context pair; the caller has asked ctx_wide_train_supported."""
    return _flow_family.log_prob_train("tnf_ctx_wide_log_prob_f32", "tnf_ctx_wide_log_prob_bwd_f32", z, params, bn_mean,
                                       bn_alpha, D, S, L, U)
