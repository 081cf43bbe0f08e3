"""Backward passes of the bijector kernels (the autograd hooks of ops.py).

Each function calls one HIP backward kernel through the C ABI (tnf_*_backward); the
activations are recomputed inside the kernel from the saved layer input, so autograd keeps
only z and the parameters alive.  Parameter gradients are reduced over the samples inside the kernels: the
shape-generic coupling / MAF kernels deterministically (fixed workgroups, partial rows added in order, a workspace
from tnf_*_backward_workspace_bytes), the narrow MFMA layer kernels with one float atomic per parameter per workgroup.
"""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _dtype_code, _grad_or_zeros, _home, _masks, _pair, _ptr, _stage, _stats, _ws


def _layer_backward(z, params, g_z, g_ld, D, ld_per_row, launch):
    """The body the coupling / affine / MAF backward share: stage (z, params), broadcast z over the parameter rows
    explicitly (its gradient is summed back over m), zeros for a gradient that did not arrive, `launch` = the entry's
    own `lib` call, results back on the devices of z and params.  log_det is (M, N), or (Mp, 1) with ld_per_row."""
    dev = _lib.require_device()
    zc, pc, pstride, Mz, Mp, M, N = _pair(z.detach(), params.detach(), dev, expanded_ok=True)
    if Mz != M:
        zc = zc.expand(M, N, D).contiguous()
    g_zo = _grad_or_zeros(g_z, (M, N, D), z.dtype, dev)
    g_l = _grad_or_zeros(g_ld, (Mp, 1) if ld_per_row else (M, N), z.dtype, dev)
    gz = torch.empty((M, N, D), dtype=z.dtype, device=dev)
    gp = torch.zeros(tuple(params.shape), dtype=params.dtype, device=dev)
    launch(dev, _dtype_code(z), zc, pc, g_zo, g_l, gz, gp, M, Mp, N, pstride)
    if Mz != M:
        gz = gz.sum(0, keepdim=True)
    return _home(gz, z.device, dev), _home(gp, params.device, dev)


def coupling_backward(z, params, z_out, g_z, g_ld, D, L, U, upper, inverse):
    def launch(dev, code, zc, pc, g_zo, g_l, gz, gp, M, Mp, N, pstride):
        if N == 0:
            return
        # with a workspace the shape-generic kernel (num_units > 16, odd D, float64 ...) reduces deterministically
        nbytes = check(lib.tnf_coupling_backward_workspace_bytes(code, M, Mp, N, D, L, U, int(upper)))
        ws, ws_bytes = _ws(nbytes, dev) if nbytes else (None, 0)
        check(lib.tnf_coupling_backward_ws(code, zc.data_ptr(), pc.data_ptr(), g_zo.data_ptr(), g_l.data_ptr(),
                                           gz.data_ptr(), gp.data_ptr(), M, Mp, N, D, L, U, int(upper), int(inverse),
                                           pstride, gp.shape[1], ws, ws_bytes, _lib.stream_ptr()))

    return _layer_backward(z, params, g_z, g_ld, D, False, launch)


def affine_backward(z, params, z_out, g_z, g_ld, D, inverse):
    def launch(dev, code, zc, pc, g_zo, g_l, gz, gp, M, Mp, N, pstride):
        check(lib.tnf_affine_backward(code, zc.data_ptr(), pc.data_ptr(), g_zo.data_ptr(), g_l.data_ptr(),
                                      gz.data_ptr(), gp.data_ptr(), M, Mp, N, D, int(inverse), pstride, gp.shape[1],
                                      _lib.stream_ptr()))

    return _layer_backward(z, params, g_z, g_ld, D, True, launch)


def maf_backward(z, params, masks, g_z, g_ld, D, L, U):
    def launch(dev, code, zc, pc, g_zo, g_l, gz, gp, M, Mp, N, pstride):
        if N == 0:
            return
        mk = _masks(masks, z.dtype, dev)
        nbytes = check(lib.tnf_maf_backward_workspace_bytes(code, M, Mp, N, D, L, U))
        ws, ws_bytes = _ws(nbytes, dev) if nbytes else (None, 0)
        check(lib.tnf_maf_backward_ws(code, zc.data_ptr(), pc.data_ptr(), mk.data_ptr(), g_zo.data_ptr(), g_l.data_ptr(),
                                      gz.data_ptr(), gp.data_ptr(), M, Mp, N, D, L, U, pstride, gp.shape[1], ws, ws_bytes,
                                      _lib.stream_ptr()))

    return _layer_backward(z, params, g_z, g_ld, D, False, launch)


def bn_apply_backward(g_z, alpha, inverse):
    if g_z is None:
        return None
    dev = _lib.require_device()
    gc = _stage(g_z, dev)
    ac = _stats(alpha, dev)
    out = torch.empty_like(gc)
    D = gc.shape[-1]
    check(lib.tnf_bn_apply_backward(_dtype_code(g_z), gc.data_ptr(), ac.data_ptr(), out.data_ptr(), gc.numel() // D, D,
                                    int(inverse), _lib.stream_ptr()))
    return _home(out, g_z.device, dev)


def bn_batch_backward(z_norm, alpha, g_zn, g_ld):
    dev = _lib.require_device()
    zc = _stage(z_norm.detach(), dev)
    D = zc.shape[-1]
    rows = zc.numel() // D
    gc = torch.zeros_like(zc) if g_zn is None else _stage(g_zn, dev).float()
    gl = None if g_ld is None else _stage(g_ld, dev).reshape(1).float()
    ac = _stats(alpha, dev)
    out = torch.empty_like(zc)
    ws_bytes = lib.tnf_bn_batch_workspace_bytes(D)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)  # a few bytes per feature: not worth the shared buffer
    check(lib.tnf_bn_batch_backward_f32(zc.data_ptr(), gc.data_ptr(), _ptr(gl), ac.data_ptr(), out.data_ptr(), rows, D,
                                        ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
    return _home(out, z_norm.device, dev)
