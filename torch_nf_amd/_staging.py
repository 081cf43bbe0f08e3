"""The staging vocabulary of ops.py and grad.py: what happens to a tensor between the caller and a `tnf_*` entry.

A wrapper is: stage the inputs (`_stage`, `_stats`, `_masks`, `_pair` for the (z, params) pair), allocate the outputs,
ONE visible `lib.tnf_*` call with `_ptr(...)` arguments (after `_ws(...)` when the entry takes a workspace), and `_home`
to hand the results back on the caller's device.  Nothing here calls the library."""
import torch

from . import _lib

_DTYPES = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _dtype_code(t):
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError("torch_nf_amd kernels take float32 or float64 tensors, not %s" % t.dtype)


def _ptr(t):
    """The pointer argument of an optional tensor."""
    return None if t is None else t.data_ptr()


def _stage(t, dev):
    """Contiguous copy/view of `t` on the compute device."""
    if t.device != dev:
        t = t.to(dev)
    return t.contiguous()


def _stats(t, dev):
    """BatchNorm statistics as contiguous float32 on the device (no-op when they already are)."""
    if t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad:
        return t
    return _stage(t.detach().float(), dev)


def _masks(masks, dtype, dev):
    """The concatenated MAF layer masks in the kernel's dtype on the device (no-op when they already are)."""
    return _stage(masks.to(dtype), dev)


def _grad_or_zeros(g, shape, dtype, dev):
    if g is None:
        return torch.zeros(shape, dtype=dtype, device=dev)
    return _stage(g, dev)


def _check3(z):
    if z.dim() != 3:
        raise ValueError("z must be (M, N, D), got shape %s" % (tuple(z.shape),))


def _rows(params, dev, expanded_ok=False):
    """(M_p, P) parameter rows with unit inner stride -> (tensor, row_stride).  A block whose rows overlap (an expanded
    single row, stride(0) == 0) is copied, unless expanded_ok: the backward kernels take it as it is, row stride 0."""
    if params.dim() != 2:
        raise ValueError("params must be (M, D_params), got shape %s" % (tuple(params.shape),))
    if params.device != dev:
        params = params.to(dev)
    if params.stride(1) != 1 or (not expanded_ok and params.shape[0] > 1 and params.stride(0) < params.shape[1]):
        params = params.contiguous()
    stride = params.stride(0) if params.shape[0] > 1 else max(params.stride(0), params.shape[1])
    return params, stride


def _pair(z, params, dev, D=None, same_dtype=False, expanded_ok=False):
    """Stage the (z, params) pair of a layer or flow entry -> (zc, pc, pstride, Mz, Mp, M, N), M the broadcast batch.
    same_dtype / D: also check params' dtype and z's last dimension."""
    if same_dtype and params.dtype != z.dtype:
        raise TypeError("z (%s) and params (%s) must have the same dtype" % (z.dtype, params.dtype))
    zc = _stage(z, dev)
    pc, pstride = _rows(params, dev, expanded_ok)
    Mz, N = zc.shape[0], zc.shape[1]
    Mp = pc.shape[0]
    if Mz != Mp and Mz != 1 and Mp != 1:
        raise RuntimeError("batch dimensions of z (%d) and params (%d) do not broadcast" % (Mz, Mp))
    if D is not None and zc.shape[2] != D:
        raise ValueError("last dimension of z (%d) must equal D (%d)" % (zc.shape[2], D))
    return zc, pc, pstride, Mz, Mp, max(Mz, Mp), N


def _home(outs, home, dev):
    """Hand results (a tensor, None, or a tuple of those) back on the caller's device.  An entry that returns on the
    compute device does not call this, and says so."""
    if home == dev:
        return outs
    if isinstance(outs, tuple):
        return tuple(None if t is None else t.to(home) for t in outs)
    return None if outs is None else outs.to(home)


_ws_cache = {}


def _workspace(nbytes, dev):
    """Grow-only scratch buffer per (device, stream); the kernels of one call are
    stream-ordered, so reuse on the same stream is safe."""
    key = (dev.index, _lib.stream_ptr())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = buf
    return buf


def _ws(nbytes, dev):
    """(pointer, size) of a workspace of at least `nbytes` (the answer of a tnf_*_workspace_bytes query): the two
    arguments of the entry.  The size is always the buffer's -- the entries only check that it suffices."""
    buf = _workspace(nbytes, dev)
    return buf.data_ptr(), buf.numel()
