"""Tensor-level wrappers of include/tnf_padbatch.h, in the staging vocabulary of _staging.py: sampling a coupling flow of
any width 2 <= D <= 63 (D != 32) with fresh batch statistics in one call -- the batch-statistics chains at the embedded
width 2H with a pad-aware fold.

`flow_padded_forward_batch_raw` (no autograd) and `flow_padded_forward_train` (one autograd node) are the entries
NormFlow routes to (families `batch_chain_padded` and `batch_train_padded`, behind the switch
`NormFlow.padded_batch_forward`); they return what ops.flow_forward_batch_raw and ops.flow_forward_train return.
`padded_batch_fold_raw` is the fold kernel alone, for the tests."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _grad_or_zeros, _home, _ptr, _stage, _ws
from .padtrain_ops import padded_width


def flow_padded_batch_supported(D, S, L, U):
    """tnf_flow_padded_batch_supported: an embedded width exists and the batch-statistics chains accept it."""
    return lib.tnf_flow_padded_batch_supported(D, S, L, U) == 1


def padded_batch_fold_raw(params_e, moments, D, affine_off, has_affine, first, eps, ldc=None):
    """tnf_flow_padded_batch_fold_f32 on embedded parameter rows (M_p, P') and moments (4H + 1,) float64 of rows in the
    embedded layout -> (mean (2H,), alpha (2H,), fold (M_p, 2, 2H), ldc (M_p,)).  Stays on the compute device."""
    W, dev, Mp = padded_width(D), params_e.device, params_e.shape[0]
    mean = torch.empty(W, dtype=torch.float32, device=dev)
    alpha = torch.empty(W, dtype=torch.float32, device=dev)
    fold = torch.empty((Mp, 2, W), dtype=torch.float32, device=dev)
    ldc = torch.zeros(Mp, dtype=torch.float32, device=dev) if ldc is None else ldc
    check(lib.tnf_flow_padded_batch_fold_f32(params_e.data_ptr(), moments.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                             fold.data_ptr(), ldc.data_ptr(), Mp, D, params_e.stride(0), affine_off,
                                             int(has_affine), int(first), float(eps), _lib.stream_ptr()))
    return mean, alpha, fold, ldc


def flow_padded_forward_batch_raw(omega, params, D, S, L, U, eps):
    """tnf_flow_padded_forward_batch_f32: NormFlow.forward with batch-statistics BatchNorm and no autograd in one call
    -> (z, sum_log_det, bn_mean (2S, D), bn_alpha (2S, D)), all on the compute device."""
    dev, oc, pc, pstride, z, sld, mean, alpha = ops._batch_prep(omega, params, D, S)
    M, N = oc.shape[0], oc.shape[1]
    Mp = pc.shape[0]
    ws, ws_bytes = _ws(check(lib.tnf_flow_padded_batch_workspace_bytes(M, Mp, N, D, S, L, U)), dev)
    check(lib.tnf_flow_padded_forward_batch_f32(oc.data_ptr(), pc.data_ptr(), z.data_ptr(), sld.data_ptr(), mean.data_ptr(),
                                                alpha.data_ptr(), M, Mp, N, D, S, L, U, pstride, float(eps), ws, ws_bytes,
                                                _lib.stream_ptr()))
    return z, sld, mean, alpha  # on the compute device: the caller carries on there


class _FlowPaddedForwardTrainFn(torch.autograd.Function):
    """NormFlow.forward with fresh batch statistics under autograd at 2 <= D <= 63 but 32
    (tnf_flow_padded_forward_train_fwd_f32 / _bwd_f32): one node for the whole stack, as ops._FlowForwardTrainFn.  The
    saved `states` (2S, M, N, 2H) and `folds` (2S, M_p, 2, 2H) are at the embedded width; omega and the parameters are
    kept at width D and embedded again by the backward.  Returns (z, sum_log_det, bn_mean, bn_alpha) on the compute
    device; the statistics are not differentiable outputs."""

    @ops._records_options
    def forward(ctx, omega, params, D, S, L, U, eps):
        dev, oc, pc, pstride, z, sld, mean, alpha = ops._batch_prep(omega, params, D, S)
        M, N = oc.shape[0], oc.shape[1]
        Mp, W = pc.shape[0], padded_width(D)
        states = torch.empty((2 * S, M, N, W), dtype=torch.float32, device=dev)
        folds = torch.empty((2 * S, Mp, 2, W), dtype=torch.float32, device=dev)
        ws, ws_bytes = _ws(check(lib.tnf_flow_padded_batch_train_workspace_bytes(M, Mp, N, D, S, L, U)), dev)
        check(lib.tnf_flow_padded_forward_train_fwd_f32(oc.data_ptr(), pc.data_ptr(), z.data_ptr(), sld.data_ptr(),
                                                        states.data_ptr(), folds.data_ptr(), mean.data_ptr(),
                                                        alpha.data_ptr(), M, Mp, N, D, S, L, U, pstride, float(eps), ws,
                                                        ws_bytes, _lib.stream_ptr()))
        ctx.save_for_backward(oc, pc, states, folds, mean, alpha)
        ctx.cfg = (D, S, L, U, pstride, omega.device, params.device, tuple(params.shape))
        ctx.mark_non_differentiable(mean, alpha)
        return z, sld, mean, alpha

    @ops._reenters_options
    def backward(ctx, g_z, g_sld, _gm, _ga):
        oc, pc, states, folds, mean, alpha = ctx.saved_tensors
        D, S, L, U, pstride, o_home, p_home, p_shape = ctx.cfg
        dev = oc.device
        M, N = oc.shape[0], oc.shape[1]
        Mp = pc.shape[0]
        gz = _stage(_grad_or_zeros(g_z, oc.shape, torch.float32, dev).float(), dev)
        gs = _stage(_grad_or_zeros(g_sld, (M, N), torch.float32, dev).float(), dev)
        go = torch.empty_like(oc) if ctx.needs_input_grad[0] else None
        gp = torch.zeros(p_shape, dtype=torch.float32, device=dev)
        ws, ws_bytes = _ws(check(lib.tnf_flow_padded_batch_train_workspace_bytes(M, Mp, N, D, S, L, U)), dev)
        check(lib.tnf_flow_padded_forward_train_bwd_f32(oc.data_ptr(), pc.data_ptr(), states.data_ptr(), folds.data_ptr(),
                                                        mean.data_ptr(), alpha.data_ptr(), gz.data_ptr(), gs.data_ptr(),
                                                        _ptr(go), gp.data_ptr(), M, Mp, N, D, S, L, U, pstride, gp.shape[1],
                                                        ws, ws_bytes, _lib.stream_ptr()))
        return _home(go, o_home, dev), _home(gp, p_home, dev), None, None, None, None, None


def flow_padded_forward_train(omega, params, D, S, L, U, eps):
    return _FlowPaddedForwardTrainFn.apply(omega, params, D, S, L, U, eps)
