"""Tensor-level wrappers of the rejection-ABC entries (include/tnf_abc.h), in the staging vocabulary of _staging.py.
A module of its own because the calls ops.py and grad.py make into the C ABI are a pinned table
(tests/ops_marshalling.json); what these wrappers hand over is pinned by tests/test_abc_host.py.

float32 only; results stay on the compute device (the drivers of lfi.py and systems.py take them home as numpy).
There is no CPU path and no composition of torch ops."""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _ptr, _stage


def _f32(**tensors):
    for name, t in tensors.items():
        if t is not None and t.dtype != torch.float32:
            raise TypeError("ABC kernels are float32 only: %s is %s" % (name, t.dtype))


def _shaped(name, t, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be %s, got shape %s" % (name, tuple(shape), tuple(t.shape)))


def _max_trials(max_trials):
    if type(max_trials) is not int or not 1 <= max_trials <= _lib.ABC_MAX_TRIALS:
        raise ValueError("max_trials must be an int in 1 .. 2^24, got %r" % (max_trials,))


def _seed(seed):
    return int(seed) & 0x7FFFFFFFFFFFFFFF


def abc_noise(seed, t, i0, n_i, j0, n_j, D):
    """tnf_abc_noise_f32: the (n_i, n_j, D) standard normals the chain kernels consume in round t for chains i0 ..
    and trials j0 .., on the compute device."""
    dev = _lib.require_device()
    omega = torch.empty((n_i, n_j, D), dtype=torch.float32, device=dev)
    if omega.numel() > 0:
        check(lib.tnf_abc_noise_f32(omega.data_ptr(), _seed(seed), t, i0, n_i, j0, n_j, D, _lib.stream_ptr()))
    return omega


def abc_smc_mat(z0, chol, bounds, x0, eps, d, max_trials, seed=0, omega=None):
    """tnf_abc_smc_mat_f32: z0 (N, D), chol (D, D), bounds (2, D), x0 (2), eps (T, 2), omega None or
    (T, N, max_trials, D) -> (zs (T, N, D), xs (T, N, 2), trials (T, N) int32) on the compute device, one launch."""
    dev = _lib.require_device()
    if type(d) is not int or lib.tnf_abc_supported(d) != 1:
        raise ValueError("the ABC kernel serves Mat(d) for 2 <= d <= %d, got d=%r" % (_lib.ABC_MAX_SMC_D, d))
    _max_trials(max_trials)
    _f32(z0=z0, chol=chol, bounds=bounds, x0=x0, eps=eps, omega=omega)
    D = d * (d + 1) // 2
    if z0.dim() != 2 or z0.shape[1] != D:
        raise ValueError("z0 must be (N, D=%d), got shape %s" % (D, tuple(z0.shape)))
    if eps.dim() != 2 or eps.shape[1] != 2:
        raise ValueError("eps must be (T, 2), got shape %s" % (tuple(eps.shape),))
    N, T = z0.shape[0], eps.shape[0]
    _shaped("chol", chol, (D, D)), _shaped("bounds", bounds, (2, D)), _shaped("x0", x0, (2,))
    if omega is not None:
        _shaped("omega", omega, (T, N, max_trials, D))
    z0c, cc, bc, xc, ec = (_stage(t, dev) for t in (z0, chol, bounds, x0, eps))
    oc = None if omega is None else _stage(omega, dev)
    zs = torch.empty((T, N, D), dtype=torch.float32, device=dev)
    xs = torch.empty((T, N, 2), dtype=torch.float32, device=dev)
    trials = torch.empty((T, N), dtype=torch.int32, device=dev)
    if N * T > 0:
        check(lib.tnf_abc_smc_mat_f32(z0c.data_ptr(), cc.data_ptr(), bc.data_ptr(), xc.data_ptr(), ec.data_ptr(), _ptr(oc),
                                      zs.data_ptr(), xs.data_ptr(), trials.data_ptr(), _seed(seed), N, T, d, max_trials,
                                      _lib.stream_ptr()))
    return zs, xs, trials


def abc_propose(mu, chol, bounds, M, max_trials, seed=0, omega=None):
    """tnf_abc_propose_f32: M truncated-Gaussian draws; mu (1, D) or (M, D), chol (D, D), bounds (2, D), omega None or
    (M, max_trials, D) -> (z (M, D), trials (M) int32) on the compute device."""
    dev = _lib.require_device()
    _max_trials(max_trials)
    _f32(mu=mu, chol=chol, bounds=bounds, omega=omega)
    if mu.dim() != 2 or mu.shape[0] not in (1, M) or not 1 <= mu.shape[1] <= _lib.ABC_MAX_D:
        raise ValueError("mu must be (1, D) or (M=%d, D) with 1 <= D <= %d, got shape %s" % (M, _lib.ABC_MAX_D,
                                                                                           tuple(mu.shape)))
    D = mu.shape[1]
    _shaped("chol", chol, (D, D)), _shaped("bounds", bounds, (2, D))
    if omega is not None:
        _shaped("omega", omega, (M, max_trials, D))
    mc, cc, bc = (_stage(t, dev) for t in (mu, chol, bounds))
    oc = None if omega is None else _stage(omega, dev)
    z = torch.empty((M, D), dtype=torch.float32, device=dev)
    trials = torch.empty((M,), dtype=torch.int32, device=dev)
    if M > 0:
        check(lib.tnf_abc_propose_f32(mc.data_ptr(), cc.data_ptr(), bc.data_ptr(), _ptr(oc), z.data_ptr(), trials.data_ptr(),
                                      _seed(seed), M, mu.shape[0], D, max_trials, _lib.stream_ptr()))
    return z, trials
