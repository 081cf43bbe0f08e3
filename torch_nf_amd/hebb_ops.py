"""Tensor-level wrappers of the Hebbian learning-rule simulator (include/tnf_hebb.h), in the staging vocabulary of
_staging.py, like abc_ops.py.  What these wrappers hand to the library is pinned by tests/test_hebb_host.py.

float32 only; results stay on the compute device and nothing here synchronises, so both calls can be captured in a HIP
graph (pass the draw index as the device tensor `t_dev` and increment it inside the captured step).  There is no CPU
path and no composition of torch ops."""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _ptr, _stage


def _f32(**tensors):
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError("the Hebbian simulator is float32 only: %s is %s" % (name, t.dtype))


def _seed(seed):
    return int(seed) & 0x7FFFFFFFFFFFFFFF


def _counter(t_dev, dev):
    """The optional device word that holds the draw index: one int64 on the compute device, handed over as it is."""
    if t_dev is None:
        return None
    if t_dev.dtype != torch.int64 or t_dev.numel() != 1 or t_dev.device != dev:
        raise ValueError("t_dev must be one int64 on the compute device, got %s %s on %s"
                         % (t_dev.dtype, tuple(t_dev.shape), t_dev.device))
    return t_dev


def _n(n):
    if type(n) is not int or lib.tnf_hebb_supported(n) != 1:
        raise ValueError("the Hebbian simulator serves 1 <= n <= %d neurons, got n=%r" % (_lib.HEBB_MAX_N, n))


def hebb_noise(seed, t, i0, n_i, j0, n_j, n, t_dev=None):
    """tnf_hebb_noise_f32: the (n_j, n_i, n) standard normals the simulator consumes in draw t for steps j0 .. and
    simulations i0 .., on the compute device."""
    dev = _lib.require_device()
    _n(n)
    td = _counter(t_dev, dev)
    omega = torch.empty((n_j, n_i, n), dtype=torch.float32, device=dev)
    if omega.numel() > 0:
        check(lib.tnf_hebb_noise_f32(omega.data_ptr(), _ptr(td), _seed(seed), t, i0, n_i, j0, n_j, n, _lib.stream_ptr()))
    return omega


def hebb_simulate(z, x, w0, n_steps, sigma_eps, seed=0, t=0, i0=0, j0=0, eps=None, traj=False, t_dev=None):
    """tnf_hebb_simulate_f32: z (N, 4) = (alpha, beta, theta_x, b), x (N_x, n) the shared inputs, w0 (n,), (1, n) or
    (N, n) the starting state, eps None (in-kernel stream) or (n_steps, N, n) standard normals -> w (N, n) after n_steps
    steps, on the compute device; with traj=True (w, traj (n_steps, N, n)), the state after each step.  Step s uses row
    (j0 + s) mod N_x of x and the normals of (seed, t, i0 + i, j0 + s); t_dev: one int64 on the device read in place
    of t."""
    dev = _lib.require_device()
    _f32(z=z, x=x, w0=w0, eps=eps)
    if z.dim() != 2 or z.shape[1] != 4:
        raise ValueError("z must be (N, 4), got shape %s" % (tuple(z.shape),))
    if x.dim() != 2 or x.shape[0] < 1:
        raise ValueError("x must be (N_x >= 1, n), got shape %s" % (tuple(x.shape),))
    N, (N_x, n) = z.shape[0], x.shape
    _n(n)
    if w0.dim() == 1:
        w0 = w0[None, :]
    if w0.dim() != 2 or w0.shape[1] != n or w0.shape[0] not in (1, N):
        raise ValueError("w0 must be (n,), (1, n) or (N, n) with N=%d, n=%d, got shape %s" % (N, n, tuple(w0.shape)))
    if type(n_steps) is not int or n_steps < 0:
        raise ValueError("n_steps must be a non-negative int, got %r" % (n_steps,))
    sigma_eps = float(sigma_eps)
    if not sigma_eps >= 0.0:
        raise ValueError("sigma_eps must be >= 0, got %r" % (sigma_eps,))
    if eps is not None and tuple(eps.shape) != (n_steps, N, n):
        raise ValueError("eps must be %s, got shape %s" % ((n_steps, N, n), tuple(eps.shape)))
    td = _counter(t_dev, dev)
    zc, xc, wc = (_stage(v, dev) for v in (z, x, w0))
    ec = None if eps is None else _stage(eps, dev)
    if n_steps == 0:  # the library launches nothing here: the result is the w0 rows
        w = wc.expand(N, n).clone()
    else:
        w = torch.empty((N, n), dtype=torch.float32, device=dev)
    tr = torch.empty((n_steps, N, n), dtype=torch.float32, device=dev) if traj else None
    if N * n_steps > 0:
        check(lib.tnf_hebb_simulate_f32(zc.data_ptr(), xc.data_ptr(), wc.data_ptr(), _ptr(ec), w.data_ptr(), _ptr(tr),
                                        _ptr(td), _seed(seed), t, i0, N, wc.shape[0], n, N_x, j0, n_steps, sigma_eps,
                                        _lib.stream_ptr()))
    return (w, tr) if traj else w
