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

`HebbLearn` is the exception: the simulator of notebooks/LFI_learning_rules.ipynb survives in the snapshot (cell 8), and
tests/golden/hebb.npz pins this package's arithmetic to it.
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


class HebbLearn(object):
    """The Hebbian learning-rule problem of the reference's notebooks/LFI_learning_rules.ipynb: parameters
    z = (alpha, beta, theta_x, b), data x = the weights of `num_neurons` neurons after `num_passes` passes over `N_x`
    shared inputs under `hebb` (cell 8), simulated by the HIP kernel of include/tnf_hebb.h.  Unlike the rest of this
    module this one is pinned to the reference: tests/golden/hebb.npz holds the notebook function's own outputs.

    `.D = 4`, `.D_x = num_neurons`, `.lb` / `.ub` / `.support_layer = ToInterval(4, lb, ub)` as in cell 4.  `.x`
    (N_x, n) is drawn as cell 4 draws it -- Sigma ~ inverse-Wishart(df = 5 n, scale = df I), x ~ N(0, Sigma) -- through
    exponential_families._inv_wishart (no scipy at run time): the same distribution, NOT the same stream as
    scipy.stats under one np.random.seed.  `.w0 ~ N(0, 1)`.  `seed` keys the simulator's noise stream (None: one
    draw from np.random, so np.random.seed governs the whole system).

    The prior is `SNPE_prior` round 1 (cell 13): alpha, beta log-uniform on [1e-5, 1e-1], theta_x uniform on (-3, 3),
    b uniform on (1, 20).  `log_prior` is the density of that draw, 1 / (z ln10 4) per log-uniform coordinate; the
    notebook's `p_z = ln(10) z` is not a density (and its loss never uses it): a deliberate deviation."""

    PRIOR_LOG10 = (-5.0, -1.0)   # alpha, beta: 10 ** uniform
    PRIOR_THETA = (-3.0, 3.0)
    PRIOR_B = (1.0, 20.0)

    def __init__(self, num_neurons=20, N_x=50, num_passes=2, sigma_eps=1e-4, seed=None):
        from .bijectors import ToInterval
        from .exponential_families import _inv_wishart

        if type(num_neurons) is not int or not 1 <= num_neurons <= 64:
            raise ValueError("num_neurons must be an int in 1 .. 64 (include/tnf_hebb.h), got %r" % (num_neurons,))
        if type(N_x) is not int or N_x < 1 or type(num_passes) is not int or num_passes < 1:
            raise ValueError("N_x and num_passes must be positive ints.")
        if not float(sigma_eps) >= 0.0:
            raise ValueError("sigma_eps must be >= 0, got %r" % (sigma_eps,))
        self.D = 4
        self.D_x = num_neurons
        self.num_neurons = num_neurons
        self.N_x = N_x
        self.num_passes = num_passes
        self.n_steps = num_passes * N_x
        self.sigma_eps = float(sigma_eps)
        self.lb = np.array([1e-6, 1e-6, -4.0, 0.0])
        self.ub = np.array([2e-1, 2e-1, 4.0, 20.0])
        self.support_layer = ToInterval(self.D, self.lb, self.ub)
        Sigma = _inv_wishart(1, num_neurons, 5 * num_neurons)[0]
        self.x = np.random.multivariate_normal(np.zeros(num_neurons), Sigma, N_x)
        self.w0 = np.random.normal(0.0, 1.0, (num_neurons,))
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self.prior = _BoxPrior(self)
        self._t = 0          # draw index of the next simulate() call
        self._dev = None     # (device, x, w0) float32 copies for the kernel
        self._bounds_key, self._bounds = None, None        # log_prior: the prior box on the device of its argument
        self._prior_key, self._prior_dev = None, None      # sample_prior_device: the box's corner and widths
        self._prior_lo = np.array([self.PRIOR_LOG10[0], self.PRIOR_LOG10[0], self.PRIOR_THETA[0], self.PRIOR_B[0]])
        self._prior_hi = np.array([self.PRIOR_LOG10[1], self.PRIOR_LOG10[1], self.PRIOR_THETA[1], self.PRIOR_B[1]])

    # ---- the prior ----------------------------------------------------------------------------------------------------
    def sample_prior(self, N):
        """(N, 4) float64 from np.random, in the notebook's order of draws (alpha, beta, theta_x, b)."""
        cols = [np.random.uniform(lo, hi, (N,)) for lo, hi in zip(self._prior_lo, self._prior_hi)]
        cols[0], cols[1] = 10.0 ** cols[0], 10.0 ** cols[1]
        return np.stack(cols, axis=1)

    def _log_prior_const(self):
        """log of: 1 / (ln10 * 4) twice, 1 / 6, 1 / 19 -- the density is this constant over alpha * beta."""
        width = self._prior_hi - self._prior_lo
        return float(-2.0 * np.log(np.log(10.0)) - np.sum(np.log(width)))

    def log_prior(self, z):
        """log density of the prior draw, -inf outside its box; z (..., 4) numpy or torch."""
        c = self._log_prior_const()
        lo = np.array([10.0 ** self._prior_lo[0], 10.0 ** self._prior_lo[1], self._prior_lo[2], self._prior_lo[3]])
        hi = np.array([10.0 ** self._prior_hi[0], 10.0 ** self._prior_hi[1], self._prior_hi[2], self._prior_hi[3]])
        if torch.is_tensor(z):
            key = (z.dtype, z.device)  # device copies of the box are made once (and keep a step capturable)
            if self._bounds_key != key:
                self._bounds = (torch.as_tensor(lo, dtype=z.dtype, device=z.device),
                                torch.as_tensor(hi, dtype=z.dtype, device=z.device))
                self._bounds_key = key
            tlo, thi = self._bounds
            inside = ((z >= tlo) & (z <= thi)).all(-1)
            lp = c - torch.log(z[..., 0]) - torch.log(z[..., 1])
            return torch.where(inside, lp, torch.full_like(lp, -float("inf")))
        z = np.asarray(z, dtype=np.float64)
        inside = np.all((z >= lo) & (z <= hi), axis=-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            lp = c - np.log(z[..., 0]) - np.log(z[..., 1])
        return np.where(inside, lp, -np.inf)

    def sample_prior_device(self, N, generator=None):
        """(z (N, 4), log_prior (N)) float32 on the HIP device from the device RNG: no host work, capturable."""
        from . import _lib

        dev = _lib.require_device()
        key = ("prior", dev)
        if self._prior_key != key:
            self._prior_dev = (torch.as_tensor(self._prior_lo, dtype=torch.float32, device=dev),
                               torch.as_tensor(self._prior_hi - self._prior_lo, dtype=torch.float32, device=dev))
            self._prior_key = key
        lo, width = self._prior_dev
        u = torch.rand((N, 4), dtype=torch.float32, device=dev, generator=generator) * width + lo
        z = torch.cat((torch.pow(10.0, u[:, :2]), u[:, 2:]), dim=1)
        log_p = self._log_prior_const() - 2.302585092994046 * (u[:, 0] + u[:, 1])
        return z, log_p

    # ---- the simulator --------------------------------------------------------------------------------------------------
    def _device_inputs(self):
        from . import _lib

        dev = _lib.require_device()
        if self._dev is None or self._dev[0] != dev:
            self._dev = (dev, torch.as_tensor(self.x, dtype=torch.float32).to(dev).contiguous(),
                         torch.as_tensor(self.w0, dtype=torch.float32).to(dev).reshape(1, -1).contiguous())
        return self._dev

    def simulate_device(self, z, t=0, t_dev=None, traj=False):
        """z (N, 4) float32 tensor -> x (N, num_neurons) on the HIP device (with traj: (x, (n_steps, N, n))).  Draw t of
        the system's noise stream, or the draw the device word t_dev holds.  No synchronisation: capturable."""
        from . import hebb_ops

        _, x, w0 = self._device_inputs()
        return hebb_ops.hebb_simulate(z, x, w0, self.n_steps, self.sigma_eps, seed=self.seed, t=t, t_dev=t_dev, traj=traj)

    def simulate(self, z, t=None):
        """z (N, 4) numpy -> x (N, num_neurons) float64 numpy, computed on the GPU (there is no CPU path): the host
        protocol of train_APT / train_SNPE.  t None: the next draw of the system's stream (a counter the call advances),
        so that repeated calls see fresh noise."""
        if t is None:
            t, self._t = self._t, (self._t + 1) % (1 << 31)
        z = torch.as_tensor(np.ascontiguousarray(np.asarray(z, dtype=np.float32).reshape(-1, 4)))
        return self.simulate_device(z, t=t).cpu().numpy().astype(np.float64)


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
