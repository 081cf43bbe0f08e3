"""The wrapper bodies that the one-launch coupling families share, in the staging vocabulary of _staging.py: ctxflow_ops,
ctxtrain_ops, ctxsample_ops, ctxwide_ops, ctxwidesample_ops, wideflow_ops and widestream_ops are these four bodies
under their own entry names.

  log_prob_raw      tnf_*_log_prob_f32        (z, params, statistics) -> (log_prob | None, z0 | None, sum_log_det | None)
  forward_raw       tnf_*_forward_f32         (omega, params, statistics) -> (z, sum_log_det), frozen BatchNorm
  log_prob_train    the first under autograd; log_prob_bwd_raw is its backward entry alone (reversible, from z0)
  sample_train      the second under autograd; sample_bwd_raw is its backward entry alone (reversible, from z)

An entry is named by a string and resolved as `getattr(lib, name)` where it is called -- one library call per body,
visible in the body, and a `lib` replaced after import (the tests' recorders) is the one that gets called.  Three call
sites serve the four bodies: `_log_prob` and `_forward` (each also the forward half of its training pair) and `_backward`,
which both pairs' backward entries share -- their argument lists differ only in the upstream gradients, one or two,
passed as a tuple.  What belongs to one family (predicates, counters, LDS and team queries, overrides) stays in its
module.  Exact float32 arithmetic: no overflow flag, no recovery path."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _ptr, _rows, _stage, _stats


def _prep(what, z, params, bn_mean, bn_alpha, D):
    """ops._flow_prep and the check of the last dimension of z (`what`: its name in the message)."""
    prep = ops._flow_prep(z, params, bn_mean, bn_alpha)
    if prep[1].shape[2] != D:
        raise ValueError("last dimension of %s (%d) must equal D (%d)" % (what, prep[1].shape[2], D))
    return prep


def _log_prob(entry, prep, D, S, L, U, want_lp, want_z0, want_sld):
    """The one launch of a tnf_*_log_prob_f32 entry on staged operands -> (lp, z0, sld) on the compute device."""
    dev, zc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = prep
    lp, z0, sld = (ops._empty_f32(want_lp, (M, N), dev), ops._empty_f32(want_z0, (M, N, D), dev),
                   ops._empty_f32(want_sld, (M, N), dev))
    check(getattr(lib, entry)(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), _ptr(lp), _ptr(z0),
                              _ptr(sld), Mz, Mp, N, D, S, L, U, pstride, _lib.stream_ptr()))
    return lp, z0, sld


def _forward(entry, prep, D, S, L, U, shared_params):
    """The one launch of a tnf_*_forward_f32 entry on staged operands -> (z, sld) on the compute device.
    shared_params: one parameter row may serve M blocks of omega -- the whole-flow argument list (Mz, Mp, N); else the
    per-context one, (M, N), with one block per row."""
    dev, oc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = prep
    if Mz != (M if shared_params else Mp):
        raise RuntimeError("sampling needs one block of omega per parameter row (%d and %d)" % (Mz, Mp))
    z = torch.empty((M, N, D), dtype=torch.float32, device=dev)
    sld = torch.empty((M, N), dtype=torch.float32, device=dev)
    check(getattr(lib, entry)(oc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), z.data_ptr(),
                              sld.data_ptr(), *((Mz, Mp) if shared_params else (M,)), N, D, S, L, U, pstride,
                              _lib.stream_ptr()))
    return z, sld


def _backward(entry, z, pc, pstride, mean_c, alpha_c, grads, D, S, L, U, p_shape, want_gin):
    """The one launch of a backward entry on staged operands: z (M, N, D) the tensor the kernel walks back from, `grads`
    the upstream gradients in the entry's order (None: NULL) -> (g_params, g_input | None) on the compute device."""
    dev = z.device
    M, N = z.shape[0], z.shape[1]
    gin = torch.empty_like(z) if want_gin else None
    P = lib.tnf_flow_num_params(D, S, L, U)
    if N == 0:  # no sample: nothing to launch (an empty tensor has no address to pass)
        return torch.zeros(p_shape, dtype=torch.float32, device=dev), gin
    # the kernel writes every parameter slot and nothing else: only trailing columns need their zeros
    gp = torch.empty(p_shape, dtype=torch.float32, device=dev) if p_shape[1] == P else \
        torch.zeros(p_shape, dtype=torch.float32, device=dev)
    check(getattr(lib, entry)(z.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                              *[_ptr(g) for g in grads], gp.data_ptr(), _ptr(gin), M, N, D, S, L, U, pstride,
                              gp.shape[1], _lib.stream_ptr()))
    return gp, gin


def log_prob_raw(entry, z, params, bn_mean, bn_alpha, D, S, L, U, want_lp, want_z0, want_sld):
    """z (M_z, N, D), params (M_p, >= D_params) -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    prep = _prep("z", z, params, bn_mean, bn_alpha, D)
    return _home(_log_prob(entry, prep, D, S, L, U, want_lp, want_z0, want_sld), z.device, prep[0])


def forward_raw(entry, omega, params, bn_mean, bn_alpha, D, S, L, U, *, shared_params):
    """omega (M, N, D), params (M, >= D_params; or one row with shared_params) -> (z, sum_log_det), one launch."""
    prep = _prep("omega", omega, params, bn_mean, bn_alpha, D)
    return _home(_forward(entry, prep, D, S, L, U, shared_params), omega.device, prep[0])


def log_prob_bwd_raw(entry, z0, params, bn_mean, bn_alpha, g_lp, D, S, L, U, want_gz):
    """z0 (M, N, D) as the forward kept it, params (M, >= D_params) one row per context, g_lp (M, N)
    -> (g_params in params' shape, trailing columns zero; g_z (M, N, D) | None), one launch."""
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
    gp, gz = _backward(entry, zc, pc, pstride, _stats(bn_mean, dev), _stats(bn_alpha, dev), (g,), D, S, L, U,
                       tuple(params.shape), want_gz)
    return _home(gp, params.device, dev), _home(gz, z0.device, dev)


class _LogProbFn(torch.autograd.Function):
    """log_prob through `fwd_entry` (a tnf_*_log_prob_f32: one launch, z0 kept); the backward is `bwd_entry`, one launch
    from z0 -- no activations are kept.  z (M_z, N, D) with M_z = M, or M_z = 1 (one block of rows for every context) when
    z needs no gradient; params (M, >= D_params)."""

    @ops._records_options
    def forward(ctx, fwd_entry, bwd_entry, z, params, bn_mean, bn_alpha, D, S, L, U):
        prep = _prep("z", z.detach(), params.detach(), bn_mean, bn_alpha, D)
        dev, _, pc, pstride, mean_c, alpha_c, Mz, Mp, _, _ = prep
        if Mz != Mp and ctx.needs_input_grad[2]:
            raise RuntimeError("a shared block of z rows that requires grad needs a sum over contexts: not offered")
        lp, z0, _ = _log_prob(fwd_entry, prep, D, S, L, U, True, True, False)
        ctx.save_for_backward(z0, pc, mean_c, alpha_c)
        ctx.cfg = (bwd_entry, D, S, L, U, pstride, z.device, params.device, tuple(params.shape))
        return _home(lp, z.device, dev)

    @ops._reenters_options
    def backward(ctx, g_lp):
        z0, pc, mean_c, alpha_c = ctx.saved_tensors
        bwd_entry, D, S, L, U, pstride, z_home, p_home, p_shape = ctx.cfg
        dev = z0.device
        gp, gz = _backward(bwd_entry, z0, pc, pstride, mean_c, alpha_c, (_stage(g_lp.float(), dev),), D, S, L, U, p_shape,
                           ctx.needs_input_grad[2])
        return None, None, _home(gz, z_home, dev), _home(gp, p_home, dev), None, None, None, None, None, None


def log_prob_train(fwd_entry, bwd_entry, z, params, bn_mean, bn_alpha, D, S, L, U):
    """log_prob (M, N) with autograd through the pair of entries named."""
    return _LogProbFn.apply(fwd_entry, bwd_entry, z, params, bn_mean, bn_alpha, D, S, L, U)


def sample_bwd_raw(entry, z, params, bn_mean, bn_alpha, g_z, g_sld, D, S, L, U, want_go):
    """z (M, N, D) as the forward returned it, params (M, >= D_params) one row per context, g_z (M, N, D) | None,
    g_sld (M, N) | None (not both None)
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
    gp, go = _backward(entry, zc, pc, pstride, _stats(bn_mean, dev), _stats(bn_alpha, dev), (gz, gs), D, S, L, U,
                       tuple(params.shape), want_go)
    return _home(gp, params.device, dev), _home(go, z.device, dev)


class _SampleFn(torch.autograd.Function):
    """Frozen-statistics sampling through `fwd_entry` (a per-context tnf_*_forward_f32: one launch, the values of the
    family's `*_forward_raw` bit for bit); the backward is `bwd_entry`, one launch from z -- only z, the staged parameter
    rows and the statistics are kept.  omega (M, N, D), params (M, >= D_params) -> (z, sum_log_det)."""

    @ops._records_options
    def forward(ctx, fwd_entry, bwd_entry, omega, params, bn_mean, bn_alpha, D, S, L, U):
        prep = _prep("omega", omega.detach(), params.detach(), bn_mean, bn_alpha, D)
        dev, _, pc, pstride, mean_c, alpha_c = prep[:6]
        z, sld = _forward(fwd_entry, prep, D, S, L, U, shared_params=False)
        ctx.save_for_backward(z, pc, mean_c, alpha_c)
        ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None: NULL for the kernel
        ctx.cfg = (bwd_entry, D, S, L, U, pstride, omega.device, params.device, tuple(params.shape))
        if omega.device == dev:
            return z, sld
        return z.to(omega.device), sld.to(omega.device)  # the saved z stays on the compute device

    @ops._reenters_options
    def backward(ctx, g_z, g_sld):
        z, pc, mean_c, alpha_c = ctx.saved_tensors
        bwd_entry, D, S, L, U, pstride, o_home, p_home, p_shape = ctx.cfg
        if g_z is None and g_sld is None:
            return (None,) * 10
        dev = z.device
        gz = None if g_z is None else _stage(g_z.float(), dev)
        gs = None if g_sld is None else _stage(g_sld.float(), dev)
        gp, go = _backward(bwd_entry, z, pc, pstride, mean_c, alpha_c, (gz, gs), D, S, L, U, p_shape,
                           ctx.needs_input_grad[2])
        return None, None, _home(go, o_home, dev), _home(gp, p_home, dev), None, None, None, None, None, None


def sample_train(fwd_entry, bwd_entry, omega, params, bn_mean, bn_alpha, D, S, L, U):
    """(z (M, N, D), sum_log_det (M, N)) with autograd through the pair of entries named."""
    return _SampleFn.apply(fwd_entry, bwd_entry, omega, params, bn_mean, bn_alpha, D, S, L, U)
