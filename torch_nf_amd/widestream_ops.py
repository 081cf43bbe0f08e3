"""Tensor-level wrappers of include/tnf_widestream.h, in the staging vocabulary of _staging.py: a coupling flow with
17 <= num_units <= 64 at any 2 <= D <= 64 and any number of stages, the whole flow in one launch with one or two layers'
operand images streamed through LDS (csrc/flow_wide_stream.hip).

`wide_flow_stream_log_prob_raw` and `wide_flow_stream_forward_raw` are the entries NormFlow routes to (family
`wide_flow_streamed`, behind the switch `NormFlow.wide_flow_streamed`); they take and return what wideflow_ops'
entries do, and accept every shape `wide_flow_stream_supported` covers -- the resident kernel's shapes included.
No autograd: calls that need gradients keep their routes."""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _home, _ptr
from .ops import _empty_f32, _flow_prep

COUNT_LOG_PROB, COUNT_FORWARD = 0, 1  # TNF_WIDESTREAM_COUNT_*
SHIPPED_TILES = (1, 2, 4)


def wide_flow_stream_supported(D, S, L, U):
    """tnf_wide_flow_stream_supported: 2 <= D <= 64, 1 <= S <= 1024, 1 <= L <= 5, 17 <= U <= 64 and ONE layer's operand
    image with its fold constants within 150 KB of LDS."""
    return lib.tnf_wide_flow_stream_supported(D, S, L, U) == 1


def lds_bytes(D, L, U):
    """tnf_wide_flow_stream_lds_bytes: the dynamic LDS of a launch (two layers if they fit, else one; 0: no such kernel)."""
    return lib.tnf_wide_flow_stream_lds_bytes(D, L, U)


def tiles(D, S, L, U, M, N):
    """tnf_wide_flow_stream_tiles: the 16-sample tiles per wave that the rule picks for M parameter rows of N samples
    (-1: no such kernel)."""
    return lib.tnf_wide_flow_stream_tiles(D, S, L, U, M, N)


def set_tiles(T):
    """tnf_wide_flow_stream_set_tiles: force T tiles per wave (1, 2 or 4; clamped to the largest the tile shape has) for
    every later launch of the process, or 0: the rule.  Returns the previous setting."""
    return check(lib.tnf_wide_flow_stream_set_tiles(T))


def launch_counts():
    """(log_prob calls, forward calls) that reached their launch."""
    return lib.tnf_wide_flow_stream_launch_count(COUNT_LOG_PROB), lib.tnf_wide_flow_stream_launch_count(COUNT_FORWARD)


def wide_flow_stream_log_prob_raw(z, params, bn_mean, bn_alpha, D, S, L, U, want_lp=True, want_z0=False, want_sld=False):
    """tnf_wide_flow_stream_log_prob_f32: z (M_z, N, D), params (M_p, >= D_params), M_z and M_p in {1, M}
    -> (log_prob | None, z0 | None, sum_log_det | None), one launch."""
    dev, zc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = _flow_prep(z, params, bn_mean, bn_alpha)
    if zc.shape[2] != D:
        raise ValueError("last dimension of z (%d) must equal D (%d)" % (zc.shape[2], D))
    lp, z0, sld = _empty_f32(want_lp, (M, N), dev), _empty_f32(want_z0, (M, N, D), dev), _empty_f32(want_sld, (M, N), dev)
    check(lib.tnf_wide_flow_stream_log_prob_f32(zc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                                _ptr(lp), _ptr(z0), _ptr(sld), Mz, Mp, N, D, S, L, U, pstride,
                                                _lib.stream_ptr()))
    return _home((lp, z0, sld), z.device, dev)


def wide_flow_stream_forward_raw(omega, params, bn_mean, bn_alpha, D, S, L, U):
    """tnf_wide_flow_stream_forward_f32 (frozen BatchNorm): omega (M, N, D), params (M or 1, >= D_params)
    -> (z (M, N, D), sum_log_det (M, N)), one launch.  The caller forms log_q = log N(omega; 0, I) - sum_log_det."""
    dev, oc, pc, pstride, mean_c, alpha_c, Mz, Mp, M, N = _flow_prep(omega, params, bn_mean, bn_alpha)
    if oc.shape[2] != D:
        raise ValueError("last dimension of omega (%d) must equal D (%d)" % (oc.shape[2], D))
    if Mz != M:
        raise RuntimeError("sampling needs one block of omega per parameter row (%d and %d)" % (Mz, Mp))
    z_out = torch.empty((M, N, D), dtype=torch.float32, device=dev)
    sld = torch.empty((M, N), dtype=torch.float32, device=dev)
    check(lib.tnf_wide_flow_stream_forward_f32(oc.data_ptr(), pc.data_ptr(), mean_c.data_ptr(), alpha_c.data_ptr(),
                                               z_out.data_ptr(), sld.data_ptr(), Mz, Mp, N, D, S, L, U, pstride,
                                               _lib.stream_ptr()))
    return _home((z_out, sld), omega.device, dev)
