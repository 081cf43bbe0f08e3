"""Tensor-level wrappers of include/tnf_ctxsample.h, in the staging vocabulary of _staging.py: training a coupling flow
with one parameter row per context and 1 <= N <= 31 draws per context through its frozen-statistics samples -- one launch
forward (tnf_ctx_flow_forward_f32, unchanged), one launch backward (tnf_ctx_sample_bwd_f32, reversible: it rebuilds every
layer's input from the forward's output z), at every 2 <= D <= 64.

`ctx_flow_sample_train` is the autograd entry NormFlow routes to (family `train_context_sample`, behind the switch
`NormFlow.context_sample_training`).  The backward kernel alone has the `_raw` wrapper, used by tools/ctxsamplebench.py
and the tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
from . import _flow_family
from ._lib import lib

# Contexts per workgroup of the backward kernel (csrc/ctx_bwd_walk.h CTX_BWD_WAVES), one wave each: the tests' edge
# cases.  Where four contexts' LDS slices exceed 64 KB (large D x N) a workgroup serves one context with all four waves
# instead; the results are the same bits either way.
WAVES_PER_WORKGROUP = 4


def ctx_sample_supported(D, S, L, U, N):
    """tnf_ctx_sample_supported: 2 <= D <= 64, S >= 1, 1 <= L <= 3, 1 <= U <= 16 and 1 <= N <= 31."""
    return lib.tnf_ctx_sample_supported(D, S, L, U, N) == 1


def launch_count():
    """Backward calls that reached their launch."""
    return lib.tnf_ctx_sample_launch_count()


def ctx_flow_sample_bwd_raw(z, params, bn_mean, bn_alpha, g_z, g_sld, D, S, L, U, want_go=True):
    """tnf_ctx_sample_bwd_f32: z (M, N, D) as the forward returned it, params (M, >= D_params) one row per context,
    g_z (M, N, D) | None, g_sld (M, N) | None (not both None)
    -> (g_params in params' shape, trailing columns zero; g_omega (M, N, D) | None), one launch."""
    return _flow_family.sample_bwd_raw("tnf_ctx_sample_bwd_f32", z, params, bn_mean, bn_alpha, g_z, g_sld, D, S, L, U,
                                       want_go)


def ctx_flow_sample_train(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """(z (M, N, D), sum_log_det (M, N)) with autograd through the per-context pair; the caller has asked
    ctx_sample_supported and forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.sample_train("tnf_ctx_flow_forward_f32", "tnf_ctx_sample_bwd_f32", omega, params, bn_mean, bn_alpha,
                                     D, S, L, U)
