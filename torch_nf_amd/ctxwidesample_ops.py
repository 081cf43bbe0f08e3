"""Tensor-level wrappers of include/tnf_ctxwidesample.h, in the staging vocabulary of _staging.py: training a coupling
flow with 17 <= num_units <= 64, one parameter row per context and 1 <= N <= 31 draws per context through its
frozen-statistics samples -- one launch forward (tnf_ctx_wide_forward_f32, unchanged), one launch backward
(tnf_ctx_wide_sample_bwd_f32, reversible: it rebuilds every layer's input from the forward's output z), at every
2 <= D <= 64.

`ctx_wide_sample_train` is the autograd entry NormFlow routes to (family `train_context_sample_wide`, behind the switch
`NormFlow.wide_context_sample_training`).  The backward kernel alone has the `_raw` wrapper, used by
tools/ctxwidesamplebench.py and the tests.  Exact float32 arithmetic: no overflow flag, no recovery path."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _ptr, _rows, _stage, _stats

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
    dev = _lib.require_device()
    if z.dtype != torch.float32 or params.dtype != torch.float32:
        raise TypeError("the fused flow kernels are float32")
    if g_z is None and g_sld is None:
        raise ValueError("no upstream gradient: g_z and g_sld are both None")
    zc = _stage(z, dev)
    pc, pstride = _rows(params, dev)
    gz = None if g_z is None else _stage(g_z.float(), dev)
    gs = None if g_sld is None else _stage(g_sld.float(), dev)
    M, N = zc.shape[0], zc.shape[1]
    if zc.shape[2] != D:
        raise ValueError("last dimension of z (%d) must equal D (%d)" % (zc.shape[2], D))
    if (pc.shape[0] != M or (gz is not None and tuple(gz.shape) != (M, N, D))
            or (gs is not None and tuple(gs.shape) != (M, N))):
        raise RuntimeError("z %s, params %s, g_z %s and g_sld %s do not describe the same contexts"
                           % (tuple(zc.shape), tuple(pc.shape), None if gz is None else tuple(gz.shape),
                              None if gs is None else tuple(gs.shape)))
    gp, go = _backward(zc, pc, pstride, _stats(bn_mean, dev), _stats(bn_alpha, dev), gz, gs, D, S, L, U,
                       tuple(params.shape), want_go)
    return _home(gp, params.device, dev), _home(go, z.device, dev)


def _backward(z, pc, pstride, mean_c, alpha_c, gz, gs, D, S, L, U, p_shape, want_go):
    """The one launch, on staged operands -> (g_params, g_omega | None) on the compute device."""
    dev = z.device
    M, N = z.shape[0], z.shape[1]
    go = torch.empty_like(z) if want_go else None
    P = lib.tnf_flow_num_params(D, S, L, U)
    if N == 0:  # no sample: nothing to launch (an empty tensor has no address to pass)
        return torch.zeros(p_shape, dtype=torch.float32, device=dev), go
    # the kernel writes every parameter slot and nothing else: only trailing columns need their zeros
    gp = torch.empty(p_shape, dtype=torch.float32, device=dev) if p_shape[1] == P else \
        torch.zeros(p_shape, dtype=torch.float32, device=dev)
    check(lib.tnf_ctx_wide_sample_bwd_f32(z.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), _ptr(gz),
                                          _ptr(gs), gp.data_ptr(), _ptr(go), M, N, D, S, L, U, pstride, gp.shape[1],
                                          _lib.stream_ptr()))
    return gp, go


class _CtxWideSampleFn(torch.autograd.Function):
    """Frozen-statistics sampling through the wide per-context kernel (tnf_ctx_wide_forward_f32: one launch, the values
    of ctxwide_ops.ctx_wide_forward_raw bit for bit); the backward is tnf_ctx_wide_sample_bwd_f32, one launch from z --
    only z, the staged parameter rows and the statistics are kept.  omega (M, N, D), params (M, >= D_params)
    -> (z, sum_log_det)."""

    @ops._records_options
    def forward(ctx, omega, params, bn_mean, bn_alpha, D, S, L, U):
        dev, oc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = ops._flow_prep(omega.detach(), params.detach(), bn_mean,
                                                                            bn_alpha)
        if oc.shape[2] != D:
            raise ValueError("last dimension of omega (%d) must equal D (%d)" % (oc.shape[2], D))
        if Mz != Mp:
            raise RuntimeError("sampling needs one block of omega per parameter row (%d and %d)" % (Mz, Mp))
        z = torch.empty((M, N, D), dtype=torch.float32, device=dev)
        sld = torch.empty((M, N), dtype=torch.float32, device=dev)
        check(lib.tnf_ctx_wide_forward_f32(oc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                           z.data_ptr(), sld.data_ptr(), M, N, D, S, L, U, pstride, _lib.stream_ptr()))
        ctx.save_for_backward(z, pc, mean_c, alpha_c)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None: NULL for the kernel
        ctx.cfg = (D, S, L, U, pstride, omega.device, params.device, tuple(params.shape))
        if omega.device == dev:
            return z, sld
        return z.to(omega.device), sld.to(omega.device)  # the saved z stays on the compute device

    @ops._reenters_options
    def backward(ctx, g_z, g_sld):
        z, pc, mean_c, alpha_c = ctx.saved_tensors
        D, S, L, U, pstride, o_home, p_home, p_shape = ctx.cfg
        if g_z is None and g_sld is None:
            return None, None, None, None, None, None, None, None
        dev = z.device
        gz = None if g_z is None else _stage(g_z.float(), dev)
        gs = None if g_sld is None else _stage(g_sld.float(), dev)
        gp, go = _backward(z, pc, pstride, mean_c, alpha_c, gz, gs, D, S, L, U, p_shape, ctx.needs_input_grad[0])
        return _home(go, o_home, dev), _home(gp, p_home, dev), None, None, None, None, None, None


def ctx_wide_sample_train(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """(z (M, N, D), sum_log_det (M, N)) with autograd through the wide per-context pair; the caller has asked
    ctx_wide_sample_supported and forms log_q = log N(omega; 0, I) - sum_log_det."""
    return _CtxWideSampleFn.apply(omega, params, bn_mean, bn_alpha, D, S, L, U)
