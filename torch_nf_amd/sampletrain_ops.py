"""Tensor-level wrappers of include/tnf_sampletrain.h, in the staging vocabulary of _staging.py: training a coupling
flow through its samples with frozen BatchNorm statistics -- `z, log_q = nf.sample(N)`, `loss(z, log_q).backward()` --
with the existing one-launch sampling kernels forward and ONE walk kernel backward.

`flow_sample_train` is the autograd entry NormFlow routes to (family `train_sample`, behind the switch
`NormFlow.sample_training`).  `flow_sample_bwd_raw` is the C call alone, used by tools/sampletrainbench.py and the
tests."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _ptr, _rows, _stage, _stats, _ws


def flow_sample_train_supported(M, Mp, N, D, S, L, U):
    """The sampling pair: a one-launch sampling forward, the walk backward from z.  Batch conditions as
    ops.flow_train_rev_supported (per-context rows need 32 samples each)."""
    return (Mp in (1, M) and N >= 1 and (Mp == 1 or N >= 32)
            and lib.tnf_flow_sample_train_supported(D, S, L, U) == 1)


def sample_train_launch_count():
    """tnf_sampletrain_launch_count: successful backward calls that reached the walk kernel's launch."""
    return int(lib.tnf_sampletrain_launch_count())


def flow_sample_bwd_raw(zc, pc, pstride, mean_c, alpha_c, g_z, g_sld, D, S, L, U, p_shape, want_omega=False, flag=None):
    """tnf_flow_sample_bwd_f32 on staged operands (compute device, contiguous float32) -> (g_params, omega | None) on
    the compute device.  g_z / g_sld: either may be None.  flag: optional one-element int32 device tensor, the overflow
    flag."""
    dev = zc.device
    M, N = zc.shape[0], zc.shape[1]
    Mp = pc.shape[0]
    gp = torch.zeros(p_shape, dtype=torch.float32, device=dev)
    omega = torch.empty_like(zc) if want_omega else None
    ws, ws_bytes = _ws(check(lib.tnf_flow_sample_train_workspace_bytes(M, Mp, N, D, S, L, U)), dev)
    check(lib.tnf_flow_sample_bwd_f32(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), _ptr(g_z),
                                      _ptr(g_sld), gp.data_ptr(), _ptr(omega), M, Mp, N, D, S, L, U, pstride, gp.shape[1],
                                      ws, ws_bytes, _ptr(flag), _lib.stream_ptr()))
    return gp, omega


def _compose_forward(omega, params, mean, alpha, D, S, L, U):
    """The sampling pass as the per-bijector composition (one autograd op per bijector, frozen statistics) ->
    (z, sum_log_det (M, N)).  The overflow recomputation: none of those kernels has a fixed-point budget."""
    z, idx, sld = omega, 0, 0.0
    for st in range(S):
        for c, upper in ((2 * st, True), (2 * st + 1, False)):
            n = lib.tnf_coupling_num_params(D, L, U, int(upper))
            z, ld = ops.coupling(z, params[:, idx:idx + n], D, L, U, upper, False)
            idx += n
            sld = sld + ld
            z, ld = ops.bn_apply(z, mean[c], alpha[c], False)
            sld = sld + ld
        z, ld = ops.affine(z, params[:, idx:idx + 2 * D], D, False)
        idx += 2 * D
        sld = sld + ld
    return z, sld


class _FlowSampleFn(torch.autograd.Function):
    """(z, sum_log_det) of the frozen-statistics sampling pass through the one-launch inference entries
    (ops.flow_forward_raw at D = 32 / 64, ops.flow_padded_forward_raw elsewhere: the values are those of the no-autograd
    route bit for bit); the backward is ONE tnf_flow_sample_bwd_f32 call that rebuilds every layer's input from z, so no
    activations are kept.  Gradients flow to `params` only: the base draw and the statistics are constants.
    `want_log_q` (a float32 tensor draw): a third output, the log_q = log N(omega; 0, I) - sum_log_det that those kernels
    write themselves (None where the selected kernel has no such output), differentiable like the other two: its
    cotangent enters the backward as minus a cotangent of sum_log_det.

    Overflow of the backward's fixed-point accumulators (a term beyond 2^13 in units where the larger cotangent is in
    [1, 2): the kernel flags it and its gradient is NaN, never a wrapped sum).  `overflow_recovery` says what then:
      "host" (default)  the flag is read back (one synchronisation per backward); when set, the gradient is recomputed
                        through the per-bijector composition from the caller's omega.  Under a stream capture the flag
                        cannot be read and the NaN poison stands.
      "off"             no recovery: an overflowing step yields a NaN gradient."""

    overflow_recovery = "host"
    overflow_fallbacks = 0  # "host" mode: how often the composition had to take over (diagnostic)
    last_overflow_flag = None  # "host" mode: the flag tensor of the latest backward (diagnostic)

    @ops._records_options
    def forward(ctx, omega, params, bn_mean, bn_alpha, D, S, L, U, fusion, want_log_q):
        dev = _lib.require_device()
        with torch.no_grad():
            if D in (32, 64):
                z, sld, log_q = ops.flow_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U, fusion, want_log_q=True) \
                    if want_log_q else ops.flow_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U, fusion) + (None,)
            else:
                z, sld, log_q = ops.flow_padded_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U, want_log_q=True) \
                    if want_log_q else ops.flow_padded_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U) + (None,)
        pc, pstride = _rows(params.detach(), dev)
        zc = _stage(z, dev)
        ctx.save_for_backward(zc, pc, _stats(bn_mean, dev), _stats(bn_alpha, dev), omega)  # omega: the caller's tensor
        ctx.cfg = (D, S, L, U, pstride, omega.device, params.device, tuple(params.shape))  # (no copy), for recovery only
        return z, sld, log_q

    @ops._reenters_options
    def backward(ctx, g_z, g_sld, g_lq=None):
        zc, pc, mean_c, alpha_c, omega = ctx.saved_tensors
        D, S, L, U, pstride, z_home, p_home, p_shape = ctx.cfg
        dev = zc.device
        gz = None if g_z is None else _stage(g_z.float(), dev)
        gs = None if g_sld is None else _stage(g_sld.float(), dev)
        if g_lq is not None:  # log_q = base(omega) - sum_log_det
            gs = _stage(-g_lq.float(), dev) if gs is None else gs - _stage(g_lq.float(), dev)
        none = (None,) * 8
        if gz is None and gs is None:
            return (None, torch.zeros(p_shape, dtype=torch.float32, device=p_home)) + none
        cls = _FlowSampleFn
        mode = cls.overflow_recovery
        if mode == "host" and torch.cuda.is_current_stream_capturing():
            mode = "off"
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if mode == "host" else None
        gp, _ = flow_sample_bwd_raw(zc, pc, pstride, mean_c, alpha_c, gz, gs, D, S, L, U, p_shape, flag=flag)
        if mode == "host":
            cls.last_overflow_flag = flag
            if int(flag.item()) != 0:
                # a term left the fixed-point budget: the same step through the per-bijector composition
                cls.overflow_fallbacks += 1
                with torch.enable_grad():
                    p = pc.detach().requires_grad_(True)
                    z2, sld2 = _compose_forward(_stage(omega.detach(), dev), p, mean_c, alpha_c, D, S, L, U)
                    outs, grads = [], []
                    if gz is not None:
                        outs.append(z2)
                        grads.append(gz)
                    if gs is not None:
                        outs.append(sld2)
                        grads.append(gs.to(sld2.dtype).expand_as(sld2))
                    gp, = torch.autograd.grad(outs, p, grads)
                gp = gp.reshape(p_shape) if gp.shape != p_shape else gp
        return (None, _home(gp, p_home, dev)) + none


def flow_sample_train(omega, params, bn_mean, bn_alpha, D, S, L, U, fusion=_lib.FUSE_AUTO, want_log_q=False):
    """(z (M, N, D), sum_log_det (M, N)) with autograd through the sampling pair -- with want_log_q a third value, the
    kernel-written log_q (M, N) float64 or None; the caller has asked flow_sample_train_supported."""
    out = _FlowSampleFn.apply(omega, params, bn_mean, bn_alpha, D, S, L, U, fusion, want_log_q)
    return out if want_log_q else out[:2]
