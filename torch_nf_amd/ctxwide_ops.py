"""Tensor-level wrappers of include/tnf_ctxwide.h, in the staging vocabulary of _staging.py: a coupling flow with
17 <= num_units <= 64, one parameter row per context and 1 <= N <= 31 samples per context -- the whole flow in one launch
(one workgroup per context, one layer's operand image resident at a time), and log_prob under autograd as one launch each
way (the forward keeps z0; the backward is reversible), at every 2 <= D <= 64.

`ctx_wide_log_prob_raw` and `ctx_wide_forward_raw` are the entries NormFlow routes to behind the switch
`NormFlow.wide_context_rows` (family `context_rows_wide`); they return what ctxflow_ops.ctx_flow_log_prob_raw and
ctx_flow_forward_raw return.  `ctx_wide_log_prob_train` is the autograd entry behind `NormFlow.wide_context_training`
(family `train_context_wide`).  The backward kernel alone has the `_raw` wrapper, used by tools/ctxwidebench.py and the
tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _ptr, _rows, _stage, _stats
from .ops import _empty_f32, _flow_prep

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
    dev, zc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = _flow_prep(z, params, bn_mean, bn_alpha)
    if zc.shape[2] != D:
        raise ValueError("last dimension of z (%d) must equal D (%d)" % (zc.shape[2], D))
    lp, z0, sld = _empty_f32(want_lp, (M, N), dev), _empty_f32(want_z0, (M, N, D), dev), _empty_f32(want_sld, (M, N), dev)
    check(lib.tnf_ctx_wide_log_prob_f32(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), _ptr(lp),
                                        _ptr(z0), _ptr(sld), Mz, Mp, N, D, S, L, U, pstride, _lib.stream_ptr()))
    return _home((lp, z0, sld), z.device, dev)


def ctx_wide_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_ctx_wide_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    dev, oc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = _flow_prep(omega, params, bn_mean, bn_alpha)
    if oc.shape[2] != D:
        raise ValueError("last dimension of omega (%d) must equal D (%d)" % (oc.shape[2], D))
    if Mz != Mp:
        raise RuntimeError("sampling needs one block of omega per parameter row (%d and %d)" % (Mz, Mp))
    z_out = torch.empty((M, N, D), dtype=torch.float32, device=dev)
    sld = torch.empty((M, N), dtype=torch.float32, device=dev)
    check(lib.tnf_ctx_wide_forward_f32(oc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                       z_out.data_ptr(), sld.data_ptr(), M, N, D, S, L, U, pstride, _lib.stream_ptr()))
    return _home((z_out, sld), omega.device, dev)


def ctx_wide_log_prob_bwd_raw(z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U, want_gz=True):
    """tnf_ctx_wide_log_prob_bwd_f32: z0 (M, N, D) as the forward kept it, params (M, >= D_params) one row per context,
    g_lp (M, N) -> (g_params in params' shape, trailing columns zero; g_z (M, N, D) | None), one launch."""
    dev = _lib.require_device()
    if z0.dtype != torch.float32 or params.dtype != torch.float32:
        raise TypeError("the fused flow kernels are float32")
    zc = _stage(z0, dev)
    pc, pstride = _rows(params, dev)
    g = _stage(g_lp.float(), dev)
    M, N = zc.shape[0], zc.shape[1]
    if zc.shape[2] != D:
        raise ValueError("last dimension of z0 (%d) must equal D (%d)" % (zc.shape[2], D))
    if pc.shape[0] != M or tuple(g.shape) != (M, N):
        raise RuntimeError("z0 %s, params %s and g_lp %s do not describe the same contexts"
                           % (tuple(zc.shape), tuple(pc.shape), tuple(g.shape)))
    gp, gz = _backward(zc, pc, pstride, _stats(bn_mean, dev), _stats(bn_alpha, dev), g, D, S, L, U,
                       tuple(params.shape), want_gz)
    return _home(gp, params.device, dev), _home(gz, z0.device, dev)


def _backward(z0, pc, pstride, mean_c, alpha_c, g, D, S, L, U, p_shape, want_gz):
    """The one launch, on staged operands -> (g_params, g_z | None) on the compute device."""
    dev = z0.device
    M, N = z0.shape[0], z0.shape[1]
    gz = torch.empty_like(z0) if want_gz else None
    P = lib.tnf_flow_num_params(D, S, L, U)
    if N == 0:  # no sample: nothing to launch (an empty tensor has no address to pass)
        return torch.zeros(p_shape, dtype=torch.float32, device=dev), gz
    # the kernel writes every parameter slot and nothing else: only trailing columns need their zeros
    gp = torch.empty(p_shape, dtype=torch.float32, device=dev) if p_shape[1] == P else \
        torch.zeros(p_shape, dtype=torch.float32, device=dev)
    check(lib.tnf_ctx_wide_log_prob_bwd_f32(z0.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                            g.data_ptr(), gp.data_ptr(), _ptr(gz), M, N, D, S, L, U, pstride,
                                            gp.shape[1], _lib.stream_ptr()))
    return gp, gz


class _CtxWideLogProbFn(torch.autograd.Function):
    """log_prob through the wide per-context kernel (tnf_ctx_wide_log_prob_f32: one launch, z0 kept); the backward is
    tnf_ctx_wide_log_prob_bwd_f32, one launch from z0 -- no activations are kept.  z (M_z, N, D) with M_z = M, or
    M_z = 1 (one block of rows for every context) when z needs no gradient; params (M, >= D_params)."""

    @ops._records_options
    def forward(ctx, z, params, bn_mean, bn_alpha, D, S, L, U):
        dev, zc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = _flow_prep(z.detach(), params.detach(), bn_mean, bn_alpha)
        if zc.shape[2] != D:
            raise ValueError("last dimension of z (%d) must equal D (%d)" % (zc.shape[2], D))
        if Mz != Mp and ctx.needs_input_grad[0]:
            raise RuntimeError("a shared block of z rows that requires grad needs a sum over contexts: not offered")
        lp = torch.empty((M, N), dtype=torch.float32, device=dev)
        z0 = torch.empty((M, N, D), dtype=torch.float32, device=dev)
        check(lib.tnf_ctx_wide_log_prob_f32(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                            lp.data_ptr(), z0.data_ptr(), None, Mz, Mp, N, D, S, L, U, pstride,
                                            _lib.stream_ptr()))
        ctx.save_for_backward(z0, pc, mean_c, alpha_c)
        ctx.cfg = (D, S, L, U, pstride, z.device, params.device, tuple(params.shape))
        return _home(lp, z.device, dev)

    @ops._reenters_options
    def backward(ctx, g_lp):
        z0, pc, mean_c, alpha_c = ctx.saved_tensors
        D, S, L, U, pstride, z_home, p_home, p_shape = ctx.cfg
        dev = z0.device
        want_gz = ctx.needs_input_grad[0]
        gp, gz = _backward(z0, pc, pstride, mean_c, alpha_c, _stage(g_lp.float(), dev), D, S, L, U, p_shape, want_gz)
        return _home(gz, z_home, dev), _home(gp, p_home, dev), None, None, None, None, None, None


def ctx_wide_log_prob_train(z, params, bn_mean, bn_alpha, D, S, L, U):
    """log_prob (M, N) with autograd through the wide per-context pair; the caller has asked ctx_wide_train_supported."""
    return _CtxWideLogProbFn.apply(z, params, bn_mean, bn_alpha, D, S, L, U)
