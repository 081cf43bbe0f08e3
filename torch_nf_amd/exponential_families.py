"""Exponential families for exponential family networks (EFNs).

Same classes and signatures as the reference's torch_nf/exponential_families.py:10-307.  `eta` is the augmented
natural parameter (a trailing 1 where the log base measure depends on z) and `T` the sufficient statistics with
log h(z) appended likewise.  The parameter conversions, the prior draws and KL are small host-side numpy, as in the
reference; the two tensor operations of an EFN objective -- T(z) and the contraction eta . T(z) -- run in HIP kernels
(ops.ef_suffstats / ops.ef_dot).  `eta_dot_T` and `efn_loss` are additions: they evaluate the loss term without ever
forming the (M, N, D_eta) tensor T(z).  `sample_eta_device` and `KL_device` are additions too: the prior draw and the KL
diagnostic as HIP kernels (efn_ops, include/tnf_efn.h), float32 on the device and without a host synchronisation, so that
efn.train_efn keeps a whole iteration on the device; the host `sample_eta` / `KL` stay what they were.

One deliberate difference: `MVN.sample_eta` draws its inverse-Wishart covariances with numpy alone (Bartlett factor),
not with scipy, which this package does not depend on.  It consumes np.random's global state, so np.random.seed
governs it, and it samples the same distribution as the reference -- not the same random stream.
"""
import math

import numpy as np
import torch

from . import _lib, ops
from .bijectors import Bijector, ToSimplex
from .error_formatters import format_type_err_msg


class ExponentialFamily(object):
    """Base class (exponential_families.py:10-99).

    :param D: Dimensionality of the random variable.
    :type D: int
    :param support_layer: Bijector class mapping onto the family's support, or None.
    :type support_layer: type, optional
    """

    _family = None  # TNF_EF_* code of the kernels, set by the subclasses

    def __init__(self, D, support_layer=None):
        super().__init__()
        self.D = D
        self.support_layer = support_layer
        self.D_eta = self._get_D_eta()

    @property
    def D(self):
        return self.__D

    @D.setter
    def D(self, val):
        if type(val) is not int:
            raise TypeError(format_type_err_msg(self, "D", val, int))
        if val < 1:
            raise ValueError("Exponential family dimensionality must be at least 1.")
        self.__D = val

    @property
    def support_layer(self):
        return self.__support_layer

    @support_layer.setter
    def support_layer(self, val):
        if val is not None and not (isinstance(val, type) and issubclass(val, Bijector)):
            raise TypeError(format_type_err_msg(self, "support_layer", val, Bijector))
        self.__support_layer = val

    def _get_D_eta(self):
        """Dimensionality of the natural parameter eta."""
        return self.D

    def sample_eta(self, N):
        """Draw N natural parameters from the family's prior -> np.ndarray (N, D_eta)."""
        raise NotImplementedError()

    def sample_eta_device(self, N, seed=0, t=0, t_dev=None):
        """`sample_eta` on the device -> float32 tensor (N, D_eta): draw t of the counter-based stream keyed by `seed`
        (include/tnf_efn.h), NOT np.random's.  t_dev: one int64 on the device read in place of t."""
        raise NotImplementedError()

    def KL_device(self, z, log_prob, eta):
        """`KL` on the device -> float32 tensor (M,): mean_n(log_prob[m, n] - log p(z[m, n]; eta[m])) by the kernels of
        include/tnf_efn.h.  z (M, N, D) float32, log_prob (M, N) float32 or float64, eta (M, D_eta); no host
        synchronisation.  A context whose eta is not a valid natural parameter gets NaN where `KL` would raise."""
        if self._family is None:
            raise NotImplementedError()
        from . import efn_ops

        self._check_z(z)
        if not torch.is_tensor(eta):
            eta = torch.as_tensor(np.asarray(eta))
        return efn_ops.efn_kl(self._family, z.detach(), log_prob.detach(), eta.detach().float())

    def mu_to_eta(self, mu):
        """Mean parameterisation -> natural parameters (N, D_eta)."""
        raise NotImplementedError()

    def eta_to_mu(self, eta):
        """Natural parameters (N, D_eta) -> mean parameterisation."""
        raise NotImplementedError()

    def T(self, z):
        """Sufficient statistics of z (M, N, D) -> (M, N, D_eta), z's dtype, on z's device."""
        raise NotImplementedError()

    def _check_z(self, z):
        if not torch.is_tensor(z) or z.dim() != 3 or z.shape[2] != self.D:
            raise ValueError("z must be a tensor of shape (M, N, %d)" % self.D)

    def _T(self, z):
        self._check_z(z)
        return ops.ef_suffstats(z, self._family)

    def eta_dot_T(self, z, eta):
        """eta[m] . T(z[m, n]) -> (M, N), equal to torch.matmul(self.T(z), eta[:, :, None])[:, :, 0] but computed by one
        kernel that never forms T(z).  eta: torch tensor or numpy array (M, D_eta); differentiable in z and eta."""
        if self._family is None:
            raise NotImplementedError()
        self._check_z(z)
        if not torch.is_tensor(eta):
            eta = torch.as_tensor(np.asarray(eta))
        if eta.dtype != z.dtype or eta.device != z.device:
            eta = eta.to(device=z.device, dtype=z.dtype)
        return ops.ef_dot(z, eta, self._family)


def _np64(a):
    """Host float64 array of a numpy array or a (possibly device-resident, graph-attached) tensor."""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _inv_wishart(N, D, df):
    """N draws of IW(df, df * I_D): W = L L^T ~ Wishart(df, I / df) by its Bartlett factor (chi on the diagonal,
    standard normals below), Sigma = W^-1."""
    shape = 0.5 * (df - np.arange(D))
    diag = np.sqrt(2.0 * np.random.gamma(shape, 1.0, (N, D)))  # chi with df - i degrees of freedom
    L = np.tril(np.random.normal(0.0, 1.0, (N, D, D)), -1)
    idx = np.arange(D)
    L[:, idx, idx] = diag
    W = np.matmul(L, np.transpose(L, (0, 2, 1))) / df
    return np.linalg.inv(W)


class MVN(ExponentialFamily):
    """Multivariate normal in its minimal representation: T(z) = [z | upper triangle of z z^T]."""

    _family = _lib.EF_MVN

    def __init__(self, D):
        super().__init__(D, None)

    def _get_D_eta(self):
        return int(self.D + self.D * (self.D + 1) // 2)

    def sample_eta(self, N=50, sigma_mu=1., iw_df_fac=5):
        """mu_i ~ N(0, sigma_mu), Sigma ~ IW(df, df * I) with df = iw_df_fac * D -> eta (N, D_eta)."""
        mu = np.random.normal(0.0, sigma_mu, (N, self.D))
        Sigma = _inv_wishart(N, self.D, iw_df_fac * self.D)
        return self.mu_to_eta(mu, Sigma)

    def sample_eta_device(self, N=50, sigma_mu=1., iw_df_fac=5, seed=0, t=0, t_dev=None):
        """The prior of `sample_eta` drawn on the device: the precision W ~ Wishart(df, I / df) is built from its Bartlett
        factor and used as it is (`sample_eta` inverts it into Sigma and `mu_to_eta` inverts Sigma again)."""
        from . import efn_ops

        return efn_ops.efn_prior(self._family, self.D, N, iw_df_fac=iw_df_fac, sigma_mu=sigma_mu, seed=seed, t=t, t_dev=t_dev)

    def T(self, z):
        return self._T(z)

    def mu_to_eta(self, mu, Sigma):
        """mu (N, D), Sigma (N, D, D) -> eta (N, D_eta): [Sigma^-1 mu | upper triangle of -Sigma^-1 / 2, off-diagonal
        entries doubled because the minimal representation keeps one of each symmetric pair]."""
        D = self.D
        P = np.linalg.inv(np.asarray(Sigma, dtype=np.float64))
        eta1 = np.matmul(P, np.asarray(mu, dtype=np.float64)[:, :, None])[:, :, 0]
        rows, cols = np.triu_indices(D)
        eta2 = -0.5 * P[:, rows, cols] * np.where(rows == cols, 1.0, 2.0)
        return np.concatenate((eta1, eta2), axis=1)

    def _precision(self, eta):
        """-2 x the symmetrised second block of eta = Sigma^-1, and eta1."""
        eta = np.asarray(eta, dtype=np.float64)
        D = self.D
        rows, cols = np.triu_indices(D)
        A = np.zeros((eta.shape[0], D, D))
        A[:, rows, cols] = eta[:, D:]
        A = 0.5 * (A + np.transpose(A, (0, 2, 1)))
        return A, eta[:, :D]

    def eta_to_mu(self, eta):
        """eta (N, D_eta) -> mu (N, D), Sigma (N, D, D)."""
        A, eta1 = self._precision(eta)
        Sigma = -0.5 * np.linalg.inv(A)
        mu = np.matmul(Sigma, eta1[:, :, None])[:, :, 0]
        return mu, Sigma

    def KL(self, z, log_prob, eta):
        """mean_n(log_prob[m, n] - log N(z[m, n]; mu_m, Sigma_m)) -> (M,), float64."""
        z, log_prob = _np64(z), _np64(log_prob)
        mu, Sigma = self.eta_to_mu(_np64(eta))
        M = z.shape[0]
        KLs = np.zeros((M,))
        for i in range(M):
            L = np.linalg.cholesky(Sigma[i])
            y = np.linalg.solve(L, (z[i] - mu[i]).T)  # (D, N)
            log_p = -0.5 * np.sum(y * y, axis=0) - np.sum(np.log(np.diag(L))) - 0.5 * self.D * math.log(2.0 * math.pi)
            KLs[i] = np.mean(log_prob[i] - log_p)
        return KLs


class Dirichlet(ExponentialFamily):
    """Dirichlet on the simplex: T(z) = [log z | sum_i log z_i], the last entry being the log base measure."""

    _family = _lib.EF_DIRICHLET

    def __init__(self, D):
        super().__init__(D, ToSimplex)

    def _get_D_eta(self):
        return self.D + 1

    def sample_eta(self, N=50, lb=0.5, ub=2.):
        """alpha_i ~ U[lb, ub] -> eta = [alpha | 1] (N, D_eta)."""
        return self.mu_to_eta(np.random.uniform(lb, ub, (N, self.D)))

    def sample_eta_device(self, N=50, lb=0.5, ub=2., seed=0, t=0, t_dev=None):
        """The prior of `sample_eta` drawn on the device."""
        from . import efn_ops

        return efn_ops.efn_prior(self._family, self.D, N, lb=lb, ub=ub, seed=seed, t=t, t_dev=t_dev)

    def T(self, z):
        return self._T(z)

    def mu_to_eta(self, alpha):
        alpha = np.asarray(alpha)
        return np.concatenate((alpha, np.ones((alpha.shape[0], 1))), axis=1)

    def eta_to_mu(self, eta):
        return eta[:, :self.D]

    def KL(self, z, log_prob, eta):
        """mean_n(log_prob[m, n] - log Dir(z[m, n]; alpha_m)) -> (M,), float64; z is nudged off the boundary by 1e-32 and
        renormalised first."""
        z = _np64(z) + 1e-32
        z = z / np.sum(z, axis=2, keepdims=True)
        log_prob = _np64(log_prob)
        alpha = self.eta_to_mu(_np64(eta))
        M = z.shape[0]
        KLs = np.zeros((M,))
        for i in range(M):
            log_norm = math.lgamma(float(np.sum(alpha[i]))) - sum(math.lgamma(float(a)) for a in alpha[i])
            log_p = log_norm + np.sum((alpha[i] - 1.0) * np.log(z[i]), axis=1)
            KLs[i] = np.mean(log_prob[i] - log_p)
        return KLs


def efn_loss(z, log_prob, eta, family):
    """The EFN objective mean(log_q(z) - eta . T(z)) of samples z (M, N, D) with log-density log_prob (M, N) drawn for
    the natural parameters eta (M, D_eta); the contraction runs in the fused kernel (family.eta_dot_T)."""
    return torch.mean(log_prob - family.eta_dot_T(z, eta))
