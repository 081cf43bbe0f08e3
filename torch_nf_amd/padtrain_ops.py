"""Tensor-level wrappers of include/tnf_padtrain.h, in the staging vocabulary of _staging.py: training a coupling flow
of any width 2 <= D <= 63 (D != 32) through the one-kernel reversible backward at the embedded width 2H.

`flow_padded_log_prob_train` is the autograd entry NormFlow routes to (family `train_padded`, behind the switch
`NormFlow.padded_training`).  The four kernels alone have `_raw` wrappers, used by the overflow recomputation here, by
tools/padded_train_bench.py and by the tests."""
import torch

from . import _lib, ops
from ._lib import lib, check
from ._staging import _home, _ptr, _stage, _ws


def flow_padded_train_supported(M, Mp, N, D, S, L, U):
    """The padded training pair: the padded whole-flow forward that keeps z0 (width D), the reversible backward at 2H.
    Batch conditions as ops.flow_train_rev_supported (per-context rows need 32 samples each)."""
    return (Mp in (1, M) and N >= 1 and (Mp == 1 or N >= 32)
            and lib.tnf_flow_padded_train_supported(D, S, L, U) == 1)


def padded_width(D):
    """tnf_flow_padded_width: 32 for 2 <= D <= 31, 64 for 33 <= D <= 63, else 0."""
    return int(lib.tnf_flow_padded_width(D))


def embed_rows_raw(rows, D):
    """tnf_flow_padded_embed_rows_f32: (..., D) float32 rows on the device -> (..., 2H), zeros at padding.  Stays on the
    compute device."""
    W = padded_width(D)
    out = torch.empty(rows.shape[:-1] + (W,), dtype=torch.float32, device=rows.device)
    check(lib.tnf_flow_padded_embed_rows_f32(rows.data_ptr(), out.data_ptr(), rows.numel() // D, D, _lib.stream_ptr()))
    return out


def gather_rows_raw(rows, D):
    """tnf_flow_padded_gather_rows_f32: (..., 2H) -> (..., D).  Stays on the compute device."""
    out = torch.empty(rows.shape[:-1] + (D,), dtype=torch.float32, device=rows.device)
    check(lib.tnf_flow_padded_gather_rows_f32(rows.data_ptr(), out.data_ptr(), out.numel() // D, D, _lib.stream_ptr()))
    return out


def embed_params_raw(pc, pstride, mean_c, alpha_c, D, S, L, U):
    """tnf_flow_padded_embed_params_f32 on staged operands -> (params (M_p, P'), bn_mean (2S, 2H), bn_alpha (2S, 2H))."""
    W = padded_width(D)
    dev = pc.device
    pe = torch.empty((pc.shape[0], lib.tnf_flow_num_params(W, S, L, U)), dtype=torch.float32, device=dev)
    mean_e = torch.empty((2 * S, W), dtype=torch.float32, device=dev)
    alpha_e = torch.empty((2 * S, W), dtype=torch.float32, device=dev)
    check(lib.tnf_flow_padded_embed_params_f32(pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(), pe.data_ptr(),
                                               mean_e.data_ptr(), alpha_e.data_ptr(), pc.shape[0], D, S, L, U, pstride,
                                               _lib.stream_ptr()))
    return pe, mean_e, alpha_e


def gather_params_raw(g, p_shape, D, S, L, U):
    """tnf_flow_padded_gather_params_f32: gradient rows (M_p, P') -> a zero-initialised `p_shape` block, real slots only."""
    out = torch.zeros(p_shape, dtype=torch.float32, device=g.device)
    check(lib.tnf_flow_padded_gather_params_f32(g.data_ptr(), out.data_ptr(), g.shape[0], D, S, L, U, out.shape[1],
                                                _lib.stream_ptr()))
    return out


def _grad_fp32_embedded(zc, pc, pstride, mean_c, alpha_c, g, D, S, L, U, p_shape, want_gz):
    """The overflow recomputation: the per-layer fp32 pair (ops._flow_log_prob_grad_fp32) at the embedded width on the
    embedded z, its gradients gathered back to width D."""
    W = padded_width(D)
    pe, mean_e, alpha_e = embed_params_raw(pc, pstride, mean_c, alpha_c, D, S, L, U)
    gz, gp = ops._flow_log_prob_grad_fp32(embed_rows_raw(zc, D), pe, pe.shape[1], mean_e, alpha_e, g, W, S, L, U,
                                          tuple(pe.shape), want_gz)
    return (gather_rows_raw(gz, D) if want_gz else None), gather_params_raw(gp, p_shape, D, S, L, U)


class _FlowPaddedLogProbFn(torch.autograd.Function):
    """log_prob through the padded whole-flow kernel (tnf_flow_padded_log_prob_f32: one launch on the real rows, z0 kept
    at width D); the backward is tnf_flow_padded_log_prob_bwd_f32 -- embed, the reversible one-kernel backward at width
    2H, gather -- so no activations are kept.

    Overflow of the backward's fixed-point accumulators is handled as in ops._FlowLogProbRevFn, with the same three
    modes of `overflow_recovery` and the same semantics: "device" (default; the recomputation is enqueued behind the
    backward, gated on the flag on the device, gated copies replace the poison), "host" (the flag is read back, one
    synchronisation per backward; not under a capture) and "off" (an overflowing step yields NaN).  The recomputation is
    the per-layer fp32 pair at the embedded width on the embedded z.  A clear flag leaves the one-kernel result
    untouched bit for bit."""

    check_overflow = True
    overflow_recovery = "device"
    overflow_fallbacks = 0  # "host" mode: how often the fp32 pair had to take over (diagnostic)
    last_overflow_flag = None  # "device" / "host" mode: the flag tensor of the latest backward (diagnostic)

    @ops._records_options
    def forward(ctx, z, params, bn_mean, bn_alpha, D, S, L, U):
        dev, zc, pc, pstride, mean_c, alpha_c = ops._train_prep(z, params, bn_mean, bn_alpha)
        M, N = zc.shape[0], zc.shape[1]
        Mp = pc.shape[0]
        lp = torch.empty((M, N), dtype=torch.float32, device=dev)
        z0 = torch.empty_like(zc)
        ws, ws_bytes = _ws(check(lib.tnf_flow_padded_workspace_bytes(M, N, D, S, L, U)), dev)
        check(lib.tnf_flow_padded_log_prob_f32(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                               lp.data_ptr(), z0.data_ptr(), None, M, Mp, N, D, S, L, U, pstride,
                                               ws, ws_bytes, _lib.stream_ptr(), None))
        ctx.save_for_backward(z0, pc, mean_c, alpha_c, zc)  # zc: the caller's tensor (no copy), for the fallback only
        ctx.cfg = (D, S, L, U, pstride, z.device, params.device, tuple(params.shape))
        return _home(lp, z.device, dev)

    @ops._reenters_options
    def backward(ctx, g_lp):
        z0, pc, mean_c, alpha_c, zc = ctx.saved_tensors
        D, S, L, U, pstride, z_home, p_home, p_shape = ctx.cfg
        dev = z0.device
        M, N = z0.shape[0], z0.shape[1]
        Mp = pc.shape[0]
        want_gz = ctx.needs_input_grad[0]
        g = _stage(g_lp.float(), dev)
        gz = torch.empty_like(z0) if want_gz else None
        gp = torch.zeros(p_shape, dtype=torch.float32, device=dev)
        ws, ws_bytes = _ws(check(lib.tnf_flow_padded_train_workspace_bytes(M, Mp, N, D, S, L, U)), dev)
        cls = _FlowPaddedLogProbFn
        mode = cls.overflow_recovery if cls.check_overflow else "off"
        if mode != "off" and not ops.flow_train_supported(M, Mp, N, padded_width(D), S, L, U):
            mode = "off"  # no per-layer pair for this shape: the poison is all there is
        if mode == "host" and torch.cuda.is_current_stream_capturing():
            mode = "off"
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if mode != "off" else None
        check(lib.tnf_flow_padded_log_prob_bwd_f32(z0.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                                   g.data_ptr(), _ptr(gz), gp.data_ptr(), M, Mp, N, D, S, L, U, pstride,
                                                   gp.shape[1], ws, ws_bytes, _ptr(flag), _lib.stream_ptr()))
        if mode != "off":
            cls.last_overflow_flag = flag
        if mode == "host" and int(flag.item()) != 0:
            # a term left the fixed-point budget: the same step through the per-layer pair, fp32 layer kernels
            cls.overflow_fallbacks += 1
            gz, gp = _grad_fp32_embedded(zc, pc, pstride, mean_c, alpha_c, g, D, S, L, U, p_shape, want_gz)
        elif mode == "device":
            # the same recomputation, enqueued now and decided on the device (ops._FlowLogProbRevFn): the layer kernels
            # of the pair exit at once while the flag is clear; the embed and gather kernels around them are not gated
            # (they only move rows), the gated copies are
            check(lib.tnf_set_launch_gate(flag.data_ptr()))
            try:
                gz2, gp2 = _grad_fp32_embedded(zc, pc, pstride, mean_c, alpha_c, g, D, S, L, U, p_shape, want_gz)
            finally:
                check(lib.tnf_set_launch_gate(None))
            check(lib.tnf_gated_copy_f32(flag.data_ptr(), gp.data_ptr(), gp2.data_ptr(), gp.numel(), _lib.stream_ptr()))
            if gz is not None:
                check(lib.tnf_gated_copy_f32(flag.data_ptr(), gz.data_ptr(), gz2.data_ptr(), gz.numel(), _lib.stream_ptr()))
        return _home(gz, z_home, dev), _home(gp, p_home, dev), None, None, None, None, None, None


def flow_padded_log_prob_train(z, params, bn_mean, bn_alpha, D, S, L, U):
    """log_prob (M, N) with autograd through the padded training pair; the caller has asked flow_padded_train_supported."""
    return _FlowPaddedLogProbFn.apply(z, params, bn_mean, bn_alpha, D, S, L, U)
