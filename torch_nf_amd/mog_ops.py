"""Tensor-level wrappers of the mixture-of-Gaussians entries (include/tnf_mog.h), in the staging vocabulary of
_staging.py like every wrapper of ops.py, which re-exports them: `ops.mog_log_prob`, `ops.mog_log_prob_raw`,
`ops.mog_sample_raw`.  A module of its own because the calls ops.py and grad.py make into the C ABI are a pinned table
(tests/ops_marshalling.json); what these wrappers hand over is pinned by tests/test_mog_host.py.

float32 only, as the reference's MoG effectively is; there is no CPU path and no composition of torch ops."""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _check3, _grad_or_zeros, _home, _pair, _ptr, _stage, _ws
from .ops import _records_options, _reenters_options


def mog_num_params(D, K):
    n = lib.tnf_mog_num_params(D, K)
    if n < 0:
        raise ValueError("no MoG with D=%r K=%r" % (D, K))
    return n


def _f32(**tensors):
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError("MoG kernels are float32 only: %s is %s" % (name, t.dtype))


def _bounds(bounds, D, dev):
    """None, or the (2, D) float32 [lb | ub] block on the device."""
    if bounds is None:
        return None
    _f32(bounds=bounds)
    if tuple(bounds.shape) != (2, D):
        raise ValueError("bounds must be (2, D) = [lb | ub], got shape %s" % (tuple(bounds.shape),))
    return _stage(bounds.detach(), dev)


def _mog_pair(z, params, D, K, dev):
    _check3(z)
    _f32(z=z, params=params)
    if params.dim() == 2 and params.shape[1] != mog_num_params(D, K):
        raise ValueError("params has %d columns, MoG(D=%d, K=%d) has D_params=%d" % (params.shape[1], D, K,
                                                                                  mog_num_params(D, K)))
    return _pair(z, params, dev, D)


def mog_log_prob_raw(z, params, D, K, bounds=None):
    """tnf_mog_log_prob_f32: z (M_z, N, D), params (M_p, D_params) -> lp (M, N) on z's device."""
    dev = _lib.require_device()
    zc, pc, ld, Mz, Mp, M, N = _mog_pair(z, params, D, K, dev)
    bc = _bounds(bounds, D, dev)
    lp = torch.empty((M, N), dtype=torch.float32, device=dev)
    if M * N > 0:
        check(lib.tnf_mog_log_prob_f32(zc.data_ptr(), pc.data_ptr(), _ptr(bc), lp.data_ptr(), Mz, Mp, N, D, K, ld,
                                       _lib.stream_ptr()))
    return _home(lp, z.device, dev)


class _MogLogProbFn(torch.autograd.Function):
    @_records_options
    def forward(ctx, z, params, bounds, D, K):
        lp = mog_log_prob_raw(z, params, D, K, bounds)
        ctx.save_for_backward(z, params, bounds)
        ctx.shape = (D, K)
        return lp

    @_reenters_options
    def backward(ctx, g_lp):
        z, params, bounds = ctx.saved_tensors
        D, K = ctx.shape
        dev = _lib.require_device()
        zc, pc, ld, Mz, Mp, M, N = _mog_pair(z.detach(), params.detach(), D, K, dev)
        bc = _bounds(bounds, D, dev)
        g = _grad_or_zeros(g_lp, (M, N), torch.float32, dev)
        want_z = ctx.needs_input_grad[0]
        gz = torch.empty((M, N, D), dtype=torch.float32, device=dev) if want_z else None
        gp = torch.empty((Mp, params.shape[1]), dtype=torch.float32, device=dev)
        if M * N > 0:
            need = check(lib.tnf_mog_bwd_workspace_bytes(M, Mp, N, D, K))
            ws, ws_bytes = _ws(need, dev) if need else (None, 0)  # a lane or a workgroup owns the whole row: no partials
            check(lib.tnf_mog_log_prob_backward_f32(zc.data_ptr(), pc.data_ptr(), _ptr(bc), g.data_ptr(), _ptr(gz),
                                                    gp.data_ptr(), Mz, Mp, N, D, K, ld, ws, ws_bytes, _lib.stream_ptr()))
        else:
            gp.zero_()
        if want_z and Mz < M:  # one z for every context: its gradient is the sum over the contexts, in context order
            gz = gz.sum(0, keepdim=True)
        return _home(gz, z.device, dev), _home(gp, params.device, dev), None, None, None


def mog_log_prob(z, params, D, K, bounds=None):
    if torch.is_grad_enabled() and (z.requires_grad or params.requires_grad):
        return _MogLogProbFn.apply(z, params, bounds, D, K)
    return mog_log_prob_raw(z, params, D, K, bounds)


def mog_sample_raw(params, u, e1, e2, D, K, bounds=None):
    """tnf_mog_sample_f32: params (M, D_params), u (M, N), e1, e2 (M, N, D) -> (z (M, N, D), log_q (M, N)) on the compute
    device: component k = #{j : cumsum(alpha)_j <= u}, z = mu_k + U_k^-1 e1 + sqrt(0.001) e2, log_q = log_prob(z)."""
    dev = _lib.require_device()
    _check3(e1)
    _f32(params=params, u=u, e1=e1, e2=e2)
    zc, pc, ld, Mz, Mp, M, N = _mog_pair(e1, params, D, K, dev)
    if Mz != Mp or tuple(u.shape) != (M, N) or e2.shape != e1.shape:
        raise ValueError("draws must be u (M, N), e1 and e2 (M, N, D) for params (M, D_params); got %s, %s, %s for %s"
                         % (tuple(u.shape), tuple(e1.shape), tuple(e2.shape), tuple(params.shape)))
    uc, e2c, bc = _stage(u, dev), _stage(e2, dev), _bounds(bounds, D, dev)
    z = torch.empty((M, N, D), dtype=torch.float32, device=dev)
    log_q = torch.empty((M, N), dtype=torch.float32, device=dev)
    if M * N > 0:
        check(lib.tnf_mog_sample_f32(pc.data_ptr(), _ptr(bc), uc.data_ptr(), zc.data_ptr(), e2c.data_ptr(), z.data_ptr(),
                                     log_q.data_ptr(), M, N, D, K, ld, _lib.stream_ptr()))
    return z, log_q
