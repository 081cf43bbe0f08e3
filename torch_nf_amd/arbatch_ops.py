"""Tensor-level wrappers of include/tnf_arbatch.h, in the staging vocabulary of _staging.py: sampling an autoregressive
flow with FRESH batch statistics -- `nf(N)`, `cde(x, N)`, `cde.sample(eta, N, freeze_bn=False)` on a NormFlow("AR") -- as
one C call forward and one backward, in place of the per-bijector composition (MAF, bn_batch_forward's three launches,
affine, and one autograd node each).

`ar_flow_forward_batch_raw` is the no-autograd call (family `ar_batch_chain`), `ar_flow_forward_batch_train` the autograd
entry (family `ar_batch_train`); both behind the switch `NormFlow.ar_batch_forward`."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _check3, _home, _masks, _pair, _ptr, _stage, _ws

COUNT_FWD_CALLS, COUNT_FWD_KERNELS, COUNT_BWD_CALLS, COUNT_BWD_KERNELS = range(4)


def ar_flow_batch_supported(D, L, U):
    """tnf_ar_flow_batch_supported: the domain of the one-kernel AR forward (tnf_ar_flow_supported)."""
    return lib.tnf_ar_flow_batch_supported(D, L, U) == 1


def ar_flow_batch_train_supported(D, L, U):
    """tnf_ar_flow_batch_train_supported: that domain and the sampling backward's (D <= 32, L <= 3, U <= 64)."""
    return lib.tnf_ar_flow_batch_train_supported(D, L, U) == 1


def arbatch_launch_count(which):
    """tnf_arbatch_launch_count: calls that reached a launch / kernels launched, forward and backward (COUNT_*)."""
    return int(check(lib.tnf_arbatch_launch_count(which)))


def _forward(omega, params, masks, D, L, U, eps):
    """Stage, allocate, the one forward call -> (z, sld, mean, alpha, pc, pstride, mk) on the compute device."""
    _check3(omega)
    dev = _lib.require_device()
    oc, pc, pstride, Mz, Mp, M, N = _pair(omega.detach(), params.detach(), dev, D)
    if Mz != M:
        raise RuntimeError("batch statistics take one block of draws per parameter row (M_z = %d, M_p = %d)" % (Mz, Mp))
    mk = _masks(masks, torch.float32, dev)
    z = torch.empty((M, N, D), dtype=torch.float32, device=dev)
    sld = torch.empty((M, N), dtype=torch.float32, device=dev)
    mean = torch.empty((D,), dtype=torch.float32, device=dev)
    alpha = torch.empty((D,), dtype=torch.float32, device=dev)
    ws, ws_bytes = _ws(check(lib.tnf_ar_flow_forward_batch_workspace_bytes(M, Mp, N, D)), dev)
    check(lib.tnf_ar_flow_forward_batch_f32(oc.data_ptr(), pc.data_ptr(), mk.data_ptr(), z.data_ptr(), sld.data_ptr(),
                                            mean.data_ptr(), alpha.data_ptr(), M, Mp, N, D, L, U, pstride, eps, ws, ws_bytes,
                                            _lib.stream_ptr()))
    return z, sld, mean, alpha, pc, pstride, mk


def ar_flow_forward_batch_raw(omega, params, masks, D, L, U, eps):
    """tnf_ar_flow_forward_batch_f32 -> (z, sum_log_det, bn_mean (D), bn_alpha (D)) on the compute device."""
    return _forward(omega, params, masks, D, L, U, eps)[:4]


def ar_flow_batch_bwd_raw(zc, pc, pstride, mk, mean, alpha, g_z, g_sld, D, L, U, p_shape):
    """tnf_ar_flow_batch_bwd_f32 on staged operands (compute device, contiguous float32) -> g_params on the compute
    device.  g_z / g_sld: either may be None."""
    dev = zc.device
    M, N = zc.shape[0], zc.shape[1]
    Mp = pc.shape[0]
    gp = torch.zeros(p_shape, dtype=torch.float32, device=dev)
    ws, ws_bytes = _ws(check(lib.tnf_ar_flow_batch_bwd_workspace_bytes(M, Mp, N, D)), dev)
    check(lib.tnf_ar_flow_batch_bwd_f32(zc.data_ptr(), pc.data_ptr(), mk.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                        _ptr(g_z), _ptr(g_sld), gp.data_ptr(), M, Mp, N, D, L, U, pstride, gp.shape[1],
                                        ws, ws_bytes, _lib.stream_ptr()))
    return gp


class _ArFlowBatchFn(torch.autograd.Function):
    """(z, sum_log_det, bn_mean, bn_alpha) of [MAF, BatchNorm, Affine] sampled with the statistics of the batch: one
    tnf_ar_flow_forward_batch_f32 call; the backward is ONE tnf_ar_flow_batch_bwd_f32 call that rebuilds the MAF sample
    from z, gradients through the batch mean and variance included, so nothing is kept but z and the 2 D statistics.
    Gradients flow to `params` only: the base draw is a constant, the statistics are handed out detached."""

    @ops._records_options
    def forward(ctx, omega, params, masks, D, L, U, eps):
        z, sld, mean, alpha, pc, pstride, mk = _forward(omega, params, masks, D, L, U, eps)
        ctx.save_for_backward(z, pc, mk, mean, alpha)
        ctx.cfg = (D, L, U, pstride, params.device, tuple(params.shape))
        ctx.mark_non_differentiable(mean, alpha)
        return z, sld, mean, alpha

    @ops._reenters_options
    def backward(ctx, g_z, g_sld, _g_mean, _g_alpha):
        zc, pc, mk, mean, alpha = ctx.saved_tensors
        D, L, U, pstride, p_home, p_shape = ctx.cfg
        dev = zc.device
        none = (None,) * 5
        if g_z is None and g_sld is None:
            return (None, torch.zeros(p_shape, dtype=torch.float32, device=p_home)) + none
        gz = None if g_z is None else _stage(g_z.float(), dev)
        gs = None if g_sld is None else _stage(g_sld.float(), dev)
        gp = ar_flow_batch_bwd_raw(zc, pc, pstride, mk, mean, alpha, gz, gs, D, L, U, p_shape)
        return (None, _home(gp, p_home, dev)) + none


def ar_flow_forward_batch_train(omega, params, masks, D, L, U, eps):
    """(z (M, N, D), sum_log_det (M, N), bn_mean (D), bn_alpha (D)) on the compute device with autograd through the
    pair; the caller has asked ar_flow_batch_train_supported."""
    return _ArFlowBatchFn.apply(omega, params, masks, D, L, U, eps)
