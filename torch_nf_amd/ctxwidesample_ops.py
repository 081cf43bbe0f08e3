"""Tensor-level wrappers of include/tnf_ctxwidesample.h, in the staging vocabulary of _staging.py: training a coupling
flow with 17 <= num_units <= 64, one parameter row per context and 1 <= N <= 31 draws per context through its
frozen-statistics samples -- one launch forward (tnf_ctx_wide_forward_f32, unchanged), one launch backward
(tnf_ctx_wide_sample_bwd_f32, reversible: it rebuilds every layer's input from the forward's output z), at every
2 <= D <= 64.

`ctx_wide_sample_train` is the autograd entry NormFlow routes to (family `train_context_sample_wide`, behind the switch
`NormFlow.wide_context_sample_training`).  The backward kernel alone has the `_raw` wrapper, used by
tools/ctxwidesamplebench.py and the tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
from . import _flow_family
from ._lib import lib, check

TEAMS = (4, 8, 16)  # the waves of a workgroup the backward kernel is built for; one workgroup serves one context


def ctx_wide_sample_supported(D, S, L, U, N):
    """tnf_ctx_wide_sample_supported: ctx_wide_supported (the forward) and ctx_wide_train_supported (the backward: L <= 3
    and the context's slice within 150 KB of LDS)."""
    return lib.tnf_ctx_wide_sample_supported(D, S, L, U, N) == 1


def launch_count():
    """Backward calls that reached their launch."""
    return lib.tnf_ctx_wide_sample_launch_count()


def waves(D, U, N):
    """tnf_ctx_wide_sample_waves: the team the backward chooses for a shape by itself (4, 8 or 16 waves), or -1."""
    return lib.tnf_ctx_wide_sample_waves(D, U, N)


def set_waves(n):
    """tnf_ctx_wide_sample_set_waves: force a team of 4, 8 or 16 waves for every later backward of the process, or 0: the
    automatic choice again.  Returns the previous value.  The results are the same bits for every team."""
    prev = lib.tnf_ctx_wide_sample_set_waves(n)
    check(prev)
    return prev


def ctx_wide_sample_bwd_raw(z, params, bn_mean, bn_alpha, g_z, g_sld, D, S, L, U, want_go=True):
    """tnf_ctx_wide_sample_bwd_f32: z (M, N, D) as the forward returned it, params (M, >= D_params) one row per context,
    g_z (M, N, D) | None, g_sld (M, N) | None (not both None)
    -> (g_params in params' shape, trailing columns zero; g_omega (M, N, D) | None), one launch."""
    return _flow_family.sample_bwd_raw("tnf_ctx_wide_sample_bwd_f32", z, params, bn_mean, bn_alpha, g_z, g_sld, D, S, L, U,
                                       want_go)


def ctx_wide_sample_train(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """(z (M, N, D), sum_log_det (M, N)) with autograd through the wide per-context pair; the caller has asked
    ctx_wide_sample_supported and forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _flow_family.sample_train("tnf_ctx_wide_forward_f32", "tnf_ctx_wide_sample_bwd_f32", omega, params, bn_mean,
                                     bn_alpha, D, S, L, U)
