"""Tensor-level wrappers of include/tnf_arsample.h, in the staging vocabulary of _staging.py: training an autoregressive
flow through its samples -- `z, log_q = nf.sample(N)`, `loss(z, log_q).backward()` on a NormFlow("AR") -- with ONE
backward kernel in place of tnf_maf_inverse_alpha, D + 1 tnf_maf_backward launches and about 3 D elementwise ops.

`maf_sample_bwd_raw` is the bijector-level call (ops._MafFn's sampling-direction backward behind the switch
`MAF.fused_sampling_backward`); `ar_flow_sample_train` is the autograd entry NormFlow routes to (family
`ar_train_sample`, behind the switch `NormFlow.ar_sample_training`): the one-kernel inference forward, the one fused
backward for [MAF, BatchNorm, Affine] with frozen statistics."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _masks, _ptr, _rows, _stage, _stats, _ws


def maf_sample_bwd_supported(D, L, U):
    """tnf_maf_sample_bwd_supported: the domain of the matrix-pipe MAF backward (D <= 32, L <= 3, U <= 64, LDS)."""
    return lib.tnf_maf_sample_bwd_supported(D, L, U) == 1


def arsample_launch_count():
    """tnf_arsample_launch_count: successful calls of the two backward entries that reached the kernel launch."""
    return int(lib.tnf_arsample_launch_count())


def maf_sample_route_ok(z, params, D, L, U):
    """May _MafFn's sampling-direction backward be the one fused call?  float32, a supported shape, one block of samples
    per parameter row or one shared row (M_z = M), exact-f32 operands."""
    return (z.dtype == torch.float32 and params.dtype == torch.float32 and z.dim() == 3
            and params.shape[0] in (1, z.shape[0]) and ops.current_operand_precision() == "fp32"
            and maf_sample_bwd_supported(D, L, U))


def maf_sample_bwd_raw(x, params, masks, g_x, g_ld, D, L, U, want_omega=True):
    """tnf_maf_sample_bwd_f32 -> (g_omega | None, g_params) on x's / params' devices.  x (M, N, D): the sample the
    forward returned; g_x / g_ld: either may be None."""
    dev = _lib.require_device()
    xc = _stage(x.detach(), dev)
    pc, pstride = _rows(params.detach(), dev)
    mk = _masks(masks, torch.float32, dev)
    M, N = xc.shape[0], xc.shape[1]
    gx = None if g_x is None else _stage(g_x.float(), dev)
    gl = None if g_ld is None else _stage(g_ld.float(), dev)
    gp = torch.zeros(tuple(params.shape), dtype=torch.float32, device=dev)
    g_omega = torch.empty_like(xc) if want_omega else None
    check(lib.tnf_maf_sample_bwd_f32(xc.data_ptr(), pc.data_ptr(), mk.data_ptr(), _ptr(gx), _ptr(gl), _ptr(g_omega),
                                     gp.data_ptr(), M, pc.shape[0], N, D, L, U, pstride, gp.shape[1], _lib.stream_ptr()))
    return _home(g_omega, x.device, dev), _home(gp, params.device, dev)


def ar_flow_sample_bwd_raw(zc, pc, pstride, mk, mean, alpha, g_z, g_sld, D, L, U, p_shape):
    """tnf_ar_flow_sample_bwd_f32 on staged operands (compute device, contiguous float32) -> g_params on the compute
    device.  g_z / g_sld: either may be None."""
    dev = zc.device
    M, N = zc.shape[0], zc.shape[1]
    Mp = pc.shape[0]
    gp = torch.zeros(p_shape, dtype=torch.float32, device=dev)
    ws, ws_bytes = _ws(check(lib.tnf_ar_flow_sample_bwd_workspace_bytes(Mp, D)), dev)
    check(lib.tnf_ar_flow_sample_bwd_f32(zc.data_ptr(), pc.data_ptr(), mk.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                         _ptr(g_z), _ptr(g_sld), gp.data_ptr(), M, Mp, N, D, L, U, pstride, gp.shape[1],
                                         ws, ws_bytes, _lib.stream_ptr()))
    return gp


def ar_flow_sample_train_supported(M, Mp, D, L, U):
    """The sampling pair of an AR flow: the one-kernel forward (ar_flow_forward_raw), the one fused backward."""
    return Mp in (1, M) and ops.ar_flow_supported(D, L, U) and maf_sample_bwd_supported(D, L, U)


class _ArFlowSampleFn(torch.autograd.Function):
    """(z, sum_log_det) of [MAF, BatchNorm, Affine] sampling with frozen statistics through the one-kernel inference
    entry (ops.ar_flow_forward_raw without a fused support layer: the values are those of the no-autograd route bit for
    bit); the backward is ONE tnf_ar_flow_sample_bwd_f32 call that rebuilds the MAF sample from z, so nothing is kept
    but z.  Gradients flow to `params` only: the base draw and the statistics are constants."""

    @ops._records_options
    def forward(ctx, omega, params, masks, bn_mean, bn_alpha, D, L, U):
        dev = _lib.require_device()
        z, sld = ops.ar_flow_forward_raw(omega, params, masks, bn_mean, bn_alpha, D, L, U)
        pc, pstride = _rows(params.detach(), dev)
        ctx.save_for_backward(z, pc, _masks(masks, torch.float32, dev), _stats(bn_mean.reshape(-1), dev),
                              _stats(bn_alpha.reshape(-1), dev))
        ctx.cfg = (D, L, U, pstride, params.device, tuple(params.shape))
        return z, sld

    @ops._reenters_options
    def backward(ctx, g_z, g_sld):
        zc, pc, mk, mean, alpha = ctx.saved_tensors
        D, L, U, pstride, p_home, p_shape = ctx.cfg
        dev = zc.device
        none = (None,) * 6
        if g_z is None and g_sld is None:
            return (None, torch.zeros(p_shape, dtype=torch.float32, device=p_home)) + none
        gz = None if g_z is None else _stage(g_z.float(), dev)
        gs = None if g_sld is None else _stage(g_sld.float(), dev)
        gp = ar_flow_sample_bwd_raw(zc, pc, pstride, mk, mean, alpha, gz, gs, D, L, U, p_shape)
        return (None, _home(gp, p_home, dev)) + none


def ar_flow_sample_train(omega, params, masks, bn_mean, bn_alpha, D, L, U):
    """(z (M, N, D), sum_log_det (M, N)) on the compute device with autograd through the sampling pair; the caller has
    asked ar_flow_sample_train_supported."""
    return _ArFlowSampleFn.apply(omega, params, masks, bn_mean, bn_alpha, D, L, U)
