"""Tensor-level wrappers of include/tnf_ctxtrain.h, in the staging vocabulary of _staging.py: training a coupling flow
with one parameter row per context and 1 <= N <= 31 samples per context -- one launch forward (tnf_ctx_flow_log_prob_f32,
which keeps z0), one launch backward (tnf_ctx_train_log_prob_bwd_f32, reversible: it rebuilds every layer's input from
z0), at every 2 <= D <= 64.

`ctx_flow_log_prob_train` is the autograd entry NormFlow routes to (family `train_context`, behind the switch
`NormFlow.context_training`).  The backward kernel alone has the `_raw` wrapper, used by tools/ctxtrainbench.py and the
tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
from . import _flow_family
from ._lib import lib

# Contexts per workgroup of the backward kernel (csrc/ctx_bwd_walk.h CTX_BWD_WAVES), one wave each: the tests' edge cases.
# Where four contexts' LDS slices exceed 64 KB (large D x N) a workgroup serves one context with all four waves instead;
# the results are the same bits either way.
WAVES_PER_WORKGROUP = 4


def ctx_train_supported(D, S, L, U, N):
    """tnf_ctx_train_supported: 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and 1 <= N <= 31."""
    return lib.tnf_ctx_train_supported(D, S, L, U, N) == 1


def launch_count():
    """Backward calls that reached their launch."""
    return lib.tnf_ctx_train_launch_count()


def ctx_flow_log_prob_bwd_raw(z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U, want_gz=True):
    """tnf_ctx_train_log_prob_bwd_f32: z0 (M, N, D) as the forward kept it, params (M, >= D_params) one row per context,
    g_lp (M, N) -> (g_params in params' shape, trailing columns zero; g_z (M, N, D) | None), one launch."""
    return _flow_family.log_prob_bwd_raw("tnf_ctx_train_log_prob_bwd_f32", z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U,
                                         want_gz)


def ctx_flow_log_prob_train(z, params, bn_mean, bn_alpha, D, S, L, U):
    """log_prob (M, N) with autograd through the per-context pair; the caller has asked ctx_train_supported."""
    return _flow_family.log_prob_train("tnf_ctx_flow_log_prob_f32", "tnf_ctx_train_log_prob_bwd_f32", z, params, bn_mean,
                                       bn_alpha, D, S, L, U)
