"""Simulators for the likelihood-free-inference drivers (stand-in for the reference's `torch_nf.systems`,
which is NOT part of the snapshot: only call sites survive -- scripts/lfi_mat.py:23, 37 and
notebooks/LFI_mat_det_trace.ipynb cells 2, 8).  What those call sites fix: `Mat(d)` has `.D = d (d + 1) / 2`
(the notebook prints samples of shape (1, 100, 6) at d = 3), bounds `.lb` / `.ub` handed to `ToInterval`, and
`simulate(z (N, D)) -> (N, 2)` summary statistics named "det / trace".  Everything else here (the entry
ordering, the bounds, the order of the two statistics, the optional observation noise) is this package's
choice: PARITY UNPINNED.

The rejection-ABC baselines (scripts/smcabc_mat.py, notebooks/ABC-MCMC.ipynb) add three more call sites:
`GaussianProposal(Sigma, lb, ub)` -- defined in the notebook's cell 2, restated here with its draws on the HIP kernel
of include/tnf_abc.h -- and `system.prior.rvs(N)` / `.logpdf(z)` and `system.abc_accept(T_x, T_x0, eps)`, of which
again only the calls survive (cells 3, 7): PARITY UNPINNED like the rest.
"""
import numpy as np
import torch


class Mat(object):
    """Symmetric d x d matrix A(z) filled row-wise from its D = d (d + 1) / 2 free entries;
    statistics x = (det A, trace A).  Uniform prior on [lb, ub]^D."""

    def __init__(self, d, bound=2.0, noise=0.0):
        if type(d) is not int or d < 1:
            raise ValueError("Mat dimension d must be a positive int.")
        self.d = d
        self.D = d * (d + 1) // 2
        self.D_x = 2
        self.lb = -bound * np.ones(self.D)
        self.ub = bound * np.ones(self.D)
        self.noise = float(noise)
        self._iu = np.triu_indices(d)
        self.prior = _BoxPrior(self)

    def sample_prior(self, N):
        return np.random.uniform(self.lb, self.ub, (N, self.D))

    def log_prior(self, z):
        """log density of the uniform prior, -inf outside the box; z (..., D) numpy or torch."""
        vol = float(np.sum(np.log(self.ub - self.lb)))
        if torch.is_tensor(z):
            key = (z.dtype, z.device)  # device copies of the bounds are made once (and keep the step capturable)
            if getattr(self, "_bounds_key", None) != key:
                self._bounds = (torch.as_tensor(self.lb, dtype=z.dtype, device=z.device),
                                torch.as_tensor(self.ub, dtype=z.dtype, device=z.device))
                self._bounds_key = key
            lb, ub = self._bounds
            inside = ((z >= lb) & (z <= ub)).all(-1)
            return torch.where(inside, torch.full(inside.shape, -vol, dtype=z.dtype, device=z.device),
                               torch.full(inside.shape, -float("inf"), dtype=z.dtype, device=z.device))
        inside = np.all((z >= self.lb) & (z <= self.ub), axis=-1)
        return np.where(inside, -vol, -np.inf)

    def abc_accept(self, T_x, T_x0, eps):
        """|T_x - T_x0| < eps in every statistic (strict; eps has one entry per statistic): T_x (..., D_x) -> bool (...)."""
        T_x, T_x0, eps = (np.asarray(v, dtype=np.float64) for v in (T_x, T_x0, eps))
        if eps.shape != (self.D_x,):
            raise ValueError("eps must have one entry per statistic, shape (%d,), got %s" % (self.D_x, eps.shape))
        return np.all(np.abs(T_x - T_x0) < eps, axis=-1)

    def matrices(self, z):
        z = np.asarray(z, dtype=np.float64)
        A = np.zeros(z.shape[:-1] + (self.d, self.d))
        A[..., self._iu[0], self._iu[1]] = z
        A[..., self._iu[1], self._iu[0]] = z
        return A

    def simulate(self, z):
        """z (N, D) -> x (N, 2) = (det A, trace A) (+ N(0, noise^2) when noise > 0)."""
        A = self.matrices(z)
        x = np.stack((np.linalg.det(A), np.trace(A, axis1=-2, axis2=-1)), axis=-1)
        if self.noise > 0.0:
            x = x + np.random.normal(0.0, self.noise, x.shape)
        return x


class _BoxPrior(object):
    """`system.prior` of the ABC call sites: the uniform box that sample_prior / log_prior implement."""

    def __init__(self, system):
        self._system = system

    def rvs(self, N):
        return self._system.sample_prior(N)

    def logpdf(self, z):
        return self._system.log_prior(z)


class GaussianProposal(object):
    """Gaussian random-walk proposal truncated to the box (lb, ub) (notebooks/ABC-MCMC.ipynb cell 2): `.D`, `.Sigma`,
    `.lb`, `.ub`, `.L = cholesky(Sigma)`.  `rvs` draws on the GPU (tnf_abc_propose_f32: the ABC kernel with its
    simulator stage compiled out; no CPU path); `pdf` / `logpdf` are the UNtruncated density, as in the notebook, in
    closed form on the host."""

    MAX_D = 21  # include/tnf_abc.h: TNF_ABC_MAX_D

    def __init__(self, Sigma, lb, ub, max_trials=1 << 16):
        Sigma, lb, ub = (np.asarray(v, dtype=np.float64) for v in (Sigma, lb, ub))
        if lb.ndim != 1 or ub.shape != lb.shape:
            raise ValueError("lb and ub must be vectors of one length, got shapes %s and %s" % (lb.shape, ub.shape))
        self.D = lb.shape[0]
        if Sigma.shape != (self.D, self.D):
            raise ValueError("Sigma must be (D, D) = (%d, %d), got shape %s" % (self.D, self.D, Sigma.shape))
        if not np.all(lb < ub):
            raise ValueError("GaussianProposal needs lb < ub in every coordinate.")
        self.Sigma = Sigma
        self.lb = lb
        self.ub = ub
        self.L = np.linalg.cholesky(Sigma)  # LinAlgError unless Sigma is positive definite
        self.max_trials = max_trials

    def _bounds(self):
        return np.stack((self.lb, self.ub))

    def rvs(self, mu, M=1, seed=None):
        """M draws z = L omega + mu, each redrawn until lb < z < ub strictly.  mu (D,) or (1, D).  Returns (M, D);
        (D,) for a one-dimensional mu and M == 1, which is what the notebook's ABC_SMC passes and expects.  seed None:
        one draw from np.random, so np.random.seed governs the result."""
        from . import abc_ops

        mu = np.asarray(mu, dtype=np.float64)
        if mu.shape not in ((self.D,), (1, self.D)):
            raise ValueError("mu must be (D,) or (1, D) with D=%d, got shape %s" % (self.D, mu.shape))
        if self.D > self.MAX_D:
            raise ValueError("the proposal kernel serves D <= %d, got D=%d" % (self.MAX_D, self.D))
        if type(M) is not int or M < 1:
            raise ValueError("M must be a positive int.")
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))
        z, trials = abc_ops.abc_propose(f32(mu.reshape(1, self.D)), f32(self.L), f32(self._bounds()), M, self.max_trials,
                                        seed)
        if int((trials == 0).sum()) > 0:
            raise RuntimeError("GaussianProposal.rvs: no point inside the box within max_trials=%d draws" % self.max_trials)
        z = z.cpu().numpy().astype(np.float64)
        return z[0] if (mu.ndim == 1 and M == 1) else z

    def logpdf(self, z, mu):
        z, mu = np.asarray(z, dtype=np.float64), np.asarray(mu, dtype=np.float64)
        if z.shape[-1:] != (self.D,) or mu.shape[-1:] != (self.D,):
            raise ValueError("z and mu must end in D=%d, got shapes %s and %s" % (self.D, z.shape, mu.shape))
        y = np.linalg.solve(self.L, (z - mu).reshape(-1, self.D).T)  # L^-1 (z - mu), one column per point
        lp = -0.5 * (np.sum(y * y, axis=0) + self.D * np.log(2.0 * np.pi)) - np.sum(np.log(np.diag(self.L)))
        lp = lp.reshape(np.broadcast(z, mu).shape[:-1])
        return lp.reshape(())[()] if lp.size == 1 else lp

    def pdf(self, z, mu):
        return np.exp(self.logpdf(z, mu))
