"""Tensor-level wrappers of the EFN prior and KL kernels (include/tnf_efn.h), in the staging vocabulary of _staging.py,
like hebb_ops.py.  What these wrappers hand to the library is pinned by tests/test_efn_host.py.

float32 only; results stay on the compute device and nothing here synchronises, so every call can be captured in a HIP
graph (pass the draw index as the device tensor `t_dev` and increment it inside the captured step).  There is no CPU
path and no composition of torch ops: an unsupported shape raises."""
import torch

from . import _lib
from ._lib import lib, check
from ._staging import _ptr, _stage, _ws
from .hebb_ops import _counter, _seed  # the stream's seed word and its optional device draw index, as the simulator's


def _shape(family, D):
    if type(D) is not int or lib.tnf_efn_supported(family, D) != 1:
        raise ValueError("the EFN kernels serve the MVN and Dirichlet families for 1 <= D <= %d, got family=%r D=%r"
                         % (_lib.EFN_MAX_D, family, D))
    return D + D * (D + 1) // 2 if family == _lib.EF_MVN else D + 1


def _num_noise(family, D, iw_df_fac):
    if type(iw_df_fac) is not int:
        raise ValueError("iw_df_fac must be an int, got %r" % (iw_df_fac,))
    K = lib.tnf_efn_prior_num_noise(family, D, iw_df_fac)
    if K < 0:
        raise ValueError("the MVN prior needs iw_df_fac >= 1 and df = iw_df_fac * D <= %d, got iw_df_fac=%r at D=%d"
                         % (_lib.EFN_MAX_DF, iw_df_fac, D))
    return K


def _rows(M):
    if type(M) is not int or M < 0:
        raise ValueError("the number of contexts must be a non-negative int, got %r" % (M,))


def efn_prior_noise(family, D, M, iw_df_fac=5, seed=0, t=0, i0=0, t_dev=None):
    """tnf_efn_prior_noise_f32: the (M, K) normals (MVN, K = D (1 + iw_df_fac D)) or uniforms (Dirichlet, K = D) that the
    prior consumes in draw t for contexts i0 .., on the compute device."""
    dev = _lib.require_device()
    _shape(family, D)
    _rows(M)
    K = _num_noise(family, D, iw_df_fac)
    td = _counter(t_dev, dev)
    noise = torch.empty((M, K), dtype=torch.float32, device=dev)
    if M > 0:
        check(lib.tnf_efn_prior_noise_f32(noise.data_ptr(), _ptr(td), family, D, iw_df_fac, _seed(seed), t, i0, M,
                                          _lib.stream_ptr()))
    return noise


def efn_prior(family, D, M, iw_df_fac=5, sigma_mu=1.0, lb=0.5, ub=2.0, seed=0, t=0, i0=0, noise=None, t_dev=None):
    """tnf_efn_prior_f32: eta (M, D_eta) float32 on the compute device.  MVN: mu ~ N(0, sigma_mu^2), precision
    ~ Wishart(df, I / df) with df = iw_df_fac * D; Dirichlet: alpha ~ U[lb, ub], eta = [alpha | 1].  noise: None (the
    in-kernel stream of (seed, t, i0 + m)) or the (M, K) draws to consume in its place; t_dev: one int64 on the device
    read in place of t."""
    dev = _lib.require_device()
    Deta = _shape(family, D)
    _rows(M)
    K = _num_noise(family, D, iw_df_fac)
    sigma_mu, lb, ub = float(sigma_mu), float(lb), float(ub)
    if family == _lib.EF_MVN and not sigma_mu >= 0.0:
        raise ValueError("sigma_mu must be >= 0, got %r" % (sigma_mu,))
    if family == _lib.EF_DIRICHLET and not (lb <= ub and abs(lb) < float("inf") and abs(ub) < float("inf")):
        raise ValueError("lb and ub must be finite with lb <= ub, got lb=%r ub=%r" % (lb, ub))
    nc = None
    if noise is not None:
        if noise.dtype != torch.float32 or tuple(noise.shape) != (M, K):
            raise ValueError("noise must be float32 %s, got %s %s" % ((M, K), noise.dtype, tuple(noise.shape)))
        nc = _stage(noise, dev)
    td = _counter(t_dev, dev)
    eta = torch.empty((M, Deta), dtype=torch.float32, device=dev)
    if M > 0:
        check(lib.tnf_efn_prior_f32(eta.data_ptr(), _ptr(nc), _ptr(td), family, D, iw_df_fac, sigma_mu, lb, ub, _seed(seed),
                                    t, i0, M, _lib.stream_ptr()))
    return eta


def efn_kl(family, z, log_q, eta):
    """tnf_efn_kl_f32: kl[m] = mean_n(log_q[m, n] - log p(z[m, n]; eta[m])) -> (M,) float32 on the compute device.
    z (M, N >= 1, D) float32, log_q (M, N) float32 or float64, eta (M, D_eta) float32.  A context whose eta is not a valid
    natural parameter gets NaN."""
    dev = _lib.require_device()
    if z.dim() != 3:
        raise ValueError("z must be (M, N, D), got shape %s" % (tuple(z.shape),))
    M, N, D = z.shape
    Deta = _shape(family, D)
    if z.dtype != torch.float32 or eta.dtype != torch.float32:
        raise TypeError("the EFN kernels are float32 only: z is %s, eta is %s" % (z.dtype, eta.dtype))
    if log_q.dtype not in (torch.float32, torch.float64):
        raise TypeError("log_q must be float32 or float64, got %s" % (log_q.dtype,))
    if N < 1 or tuple(log_q.shape) != (M, N) or tuple(eta.shape) != (M, Deta):
        raise ValueError("need N >= 1, log_q (M, N) and eta (M, %d) for z %s, got log_q %s and eta %s"
                         % (Deta, tuple(z.shape), tuple(log_q.shape), tuple(eta.shape)))
    zc, lc, ec = (_stage(v, dev) for v in (z, log_q, eta))
    kl = torch.empty((M,), dtype=torch.float32, device=dev)
    if M > 0:
        ws, ws_bytes = _ws(lib.tnf_efn_kl_workspace_bytes(family, M, N, D), dev)
        check(lib.tnf_efn_kl_f32(zc.data_ptr(), lc.data_ptr(), _lib.F64 if lc.dtype == torch.float64 else _lib.F32,
                                 ec.data_ptr(), kl.data_ptr(), family, M, N, D, ws, ws_bytes, _lib.stream_ptr()))
    return kl
