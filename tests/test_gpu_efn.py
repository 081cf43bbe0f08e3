"""The EFN prior and KL kernels (include/tnf_efn.h) on the GPU against the float64 restatement
(tests/efn_restatement.py, tied to the reference by tests/test_efn_host.py), the families' device methods, and
efn.train_efn on top of them.

Bars.  The prior's is derived, never measured: 4 * n_terms * 2^-24 of a row's largest |eta| entry, n_terms the longest
float32 sum behind an entry (efn_restatement.eta_bar: df for a chi-square, D for a row of L L^T).  The KL's is the
project's convention (tests/test_gpu_grad.py): 4 x the largest |KL_device - KL_host| / (1 + |KL_host|) measured over the
random grid on the MI355X, the figure kept beside KL_MEASURED below; every run prints what it sees."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
import efn_restatement as R

pytestmark = pytest.mark.gpu

SEED = (11 << 32) | 77
# largest |KL_device - KL_host| / (1 + |KL_host|) over the random grid of test_kl_random_grid, MI355X: 3.25e-7 (Dirichlet,
# D = 64, N = 1: one sample, nothing averages out; the golden rows reach 1.3e-7)
KL_MEASURED = 3.3e-7
KL_BAR = 4.0 * KL_MEASURED
_seen = {"kl": 0.0}


def f32x(a):
    """float32-exact float64: what the kernel is handed is what the float64 reference sees"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C")).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ops():
    from torch_nf_amd import efn_ops

    return efn_ops


def fams():
    from torch_nf_amd import _lib

    return _lib.EF_MVN, _lib.EF_DIRICHLET


# ---- 1. the prior against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 257])
@pytest.mark.parametrize("fac", [1, 5])
@pytest.mark.parametrize("D", [1, 2, 5, 16, 64])
def test_mvn_prior_is_the_restatement_of_its_noise(D, fac, M):
    mvn, _ = fams()
    df = fac * D
    kw = dict(iw_df_fac=fac, seed=SEED, t=5, i0=3)
    noise = ops().efn_prior_noise(mvn, D, M, **kw)
    assert tuple(noise.shape) == (M, R.mvn_num_noise(D, df)) and bool(torch.isfinite(noise).all())
    eta = ops().efn_prior(mvn, D, M, sigma_mu=1.5, **kw)
    fed = ops().efn_prior(mvn, D, M, sigma_mu=1.5, noise=noise, **kw)
    assert torch.equal(eta, fed)  # the recorded noise gives the in-kernel-stream result bit for bit
    want = R.mvn_eta(host(noise), D, df, sigma_mu=1.5)
    err = np.abs(host(eta) - want).max(axis=1)
    bar = R.eta_bar(want, D, df)
    print("MVN prior D=%d df=%d M=%d: worst error / bar %.3f" % (D, df, M, float((err / bar).max())))
    assert (err <= bar).all(), (float((err / bar).max()), int(np.argmax(err / bar)))


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("D", [1, 3, 64])
def test_dirichlet_prior_is_the_restatement_of_its_noise(D, M):
    _, dirichlet = fams()
    kw = dict(seed=SEED, t=2, i0=9)
    u = ops().efn_prior_noise(dirichlet, D, M, **kw)
    assert tuple(u.shape) == (M, D) and bool((u > 0).all()) and bool((u <= 1).all())
    eta = ops().efn_prior(dirichlet, D, M, lb=0.5, ub=2.0, **kw)
    assert torch.equal(eta, ops().efn_prior(dirichlet, D, M, lb=0.5, ub=2.0, noise=u, **kw))
    want = R.dirichlet_eta(host(u), 0.5, 2.0)
    assert (np.abs(host(eta) - want).max(axis=1) <= R.eta_bar(want, D)).all()
    assert bool((eta[:, D] == 1.0).all()) and bool((eta[:, :D] >= 0.5).all()) and bool((eta[:, :D] <= 2.0).all())


@pytest.mark.parametrize("family_D", [("mvn", 5), ("mvn", 64), ("dir", 7)])
def test_prior_placement_independence(family_D):
    name, D = family_D
    fam = fams()[0 if name == "mvn" else 1]
    kw = dict(iw_df_fac=2, seed=SEED)
    full = ops().efn_prior(fam, D, 300, t=4, **kw)
    part = ops().efn_prior(fam, D, 17, t=4, i0=40, **kw)
    assert torch.equal(full[40:57], part)  # a context's draw does not depend on its place in the launch
    assert torch.equal(ops().efn_prior_noise(fam, D, 300, t=4, **kw)[40:57], ops().efn_prior_noise(fam, D, 17, t=4, i0=40, **kw))
    word = torch.full((1,), 4, dtype=torch.int64, device="cuda")
    assert torch.equal(ops().efn_prior(fam, D, 300, t=0, t_dev=word, **kw), full)  # the device word is read in place of t
    assert torch.equal(ops().efn_prior_noise(fam, D, 17, t=9, i0=40, t_dev=word, **kw),
                       ops().efn_prior_noise(fam, D, 17, t=4, i0=40, **kw))
    cols = slice(0, D)  # Dirichlet's last column is the constant 1
    for other in (ops().efn_prior(fam, D, 300, t=5, **kw), ops().efn_prior(fam, D, 300, t=4, iw_df_fac=2, seed=SEED + 1),
                  ops().efn_prior(fam, D, 300, t=4, iw_df_fac=2, seed=SEED + (1 << 32))):
        assert bool((other[:, cols] != full[:, cols]).any(dim=1).all())  # another draw index or seed: every row changes


def test_prior_distributions():
    """Means within 6 standard errors, the errors computed from M: W ~ Wishart(df, I / df) has mean I and per-entry variance
    2 / df on the diagonal, 1 / df off it; mu ~ N(0, sigma_mu^2); alpha ~ U[lb, ub].  A sample variance over n draws has
    the relative standard error sqrt((kurtosis - 1) / n): kurtosis 3 for the normal, 1.8 for the uniform."""
    from torch_nf_amd.exponential_families import MVN, Dirichlet

    M, D, fac, sigma = 8192, 5, 5, 0.7
    df = fac * D
    eta = host(MVN(D).sample_eta_device(M, sigma_mu=sigma, iw_df_fac=fac, seed=SEED))
    rows, cols = np.triu_indices(D)
    P = np.zeros((M, D, D))
    P[:, rows, cols] = -eta[:, D:]
    P = P + np.transpose(P, (0, 2, 1))
    mean = P.mean(axis=0)
    se = np.sqrt(np.where(np.eye(D) > 0, 2.0, 1.0) / df / M)
    assert (np.abs(mean - np.eye(D)) <= 6.0 * se).all(), np.abs(mean - np.eye(D)) / se
    mu = np.linalg.solve(P, eta[:, :D, None])[:, :, 0]
    n = M * D
    assert abs(mu.mean()) <= 6.0 * sigma / np.sqrt(n)
    assert abs(mu.var() - sigma ** 2) <= 6.0 * sigma ** 2 * np.sqrt(2.0 / n)
    lb, ub, Dd = 0.25, 3.0, 7
    alpha = host(Dirichlet(Dd).sample_eta_device(M, lb=lb, ub=ub, seed=SEED))[:, :Dd]
    n, var = M * Dd, (ub - lb) ** 2 / 12.0
    assert abs(alpha.mean() - 0.5 * (lb + ub)) <= 6.0 * np.sqrt(var / n)
    assert abs(alpha.var() - var) <= 6.0 * var * np.sqrt(0.8 / n)
    assert abs(alpha.mean(axis=0) - 0.5 * (lb + ub)).max() <= 6.0 * np.sqrt(var / M)


# ---- 2. KL ----------------------------------------------------------------------------------------------------------------
def kl_err(got, want):
    return float(np.max(np.abs(got - want) / (1.0 + np.abs(want))))


@pytest.mark.parametrize("D", [2, 5, 20])
@pytest.mark.parametrize("name", ["mvn", "dir"])
def test_kl_golden_rows(name, D):
    """The contexts of tests/golden/expfam.npz against the reference's own KL values (computed there in float64 from
    float64 eta; the kernel is handed eta and z rounded to float32)."""
    from torch_nf_amd.exponential_families import MVN, Dirichlet

    g = load_golden("expfam")
    k = "%s%d_" % (name, D)
    fam = (MVN if name == "mvn" else Dirichlet)(D)
    for lq in (dev(g[k + "lp"], np.float64), dev(g[k + "lp"])):
        got = fam.KL_device(dev(g[k + "z32"]), lq, dev(g[k + "eta"][:3]))
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (3,)
        err = kl_err(host(got), g[k + "KL"])
        print("golden %s D=%d log_q %s: KL error %.3e" % (name, D, lq.dtype, err))
        assert err <= KL_BAR


@functools.lru_cache(maxsize=None)
def _kl_case(name, D, M, N):
    """Inputs of one grid case, float32-exact, and the host float64 KL of them (computed once, shared, never changed)."""
    from torch_nf_amd.exponential_families import MVN, Dirichlet

    rng = np.random.RandomState(1000 * D + 10 * M + N + (0 if name == "mvn" else 7))
    if name == "mvn":
        fam = MVN(D)
        df = 5 * D
        noise = rng.normal(0.0, 1.0, (M, R.mvn_num_noise(D, df)))
        eta = f32x(R.mvn_eta(noise, D, df))
        mu, Sigma = fam.eta_to_mu(eta)
        z = f32x(mu[:, None, :] + 1.5 * rng.normal(0.0, 1.0, (M, N, D)))
    else:
        fam = Dirichlet(D)
        eta = f32x(R.dirichlet_eta(rng.uniform(0.0, 1.0, (M, D)), 0.5, 2.0))
        z = f32x(rng.dirichlet(np.ones(D), (M, N)))
        z[:, 0, 0] = 0.0  # a row holding an exact 0
        if N > 1:
            z[:, N // 2, D - 1] = 0.0
    lq = rng.normal(-10.0, 5.0, (M, N))
    want = fam.KL(z, f32x(lq), eta)
    want64 = fam.KL(z, lq, eta)
    for a in (eta, z, lq, want, want64):
        a.setflags(write=False)
    return fam, eta, z, lq, want, want64


@pytest.mark.parametrize("N", [1, 129, 1000])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("name_D", [("mvn", 1), ("mvn", 2), ("mvn", 5), ("mvn", 16), ("mvn", 63), ("mvn", 64), ("dir", 2),
                                    ("dir", 5), ("dir", 64)])
def test_kl_random_grid(name_D, M, N):
    name, D = name_D
    fam, eta, z, lq, want32, want64 = _kl_case(name, D, M, N)
    assert np.isfinite(want64).all()
    zd, ed = dev(z), dev(eta)
    for lqd, want in ((dev(lq), want32), (dev(lq, np.float64), want64)):
        got = fam.KL_device(zd, lqd, ed)
        assert got.dtype == torch.float32 and tuple(got.shape) == (M,)
        assert torch.equal(got, fam.KL_device(zd, lqd, ed))  # reproducible bit for bit
        err = kl_err(host(got), want)
        _seen["kl"] = max(_seen["kl"], err)
        print("KL %s D=%d M=%d N=%d log_q %s: error %.3e (largest so far %.3e), largest |KL| %.1f"
              % (name, D, M, N, lqd.dtype, err, _seen["kl"], float(np.abs(want).max())))
        assert err <= KL_BAR, (err, KL_BAR)


def test_kl_invalid_natural_parameter_is_nan_in_its_row_only():
    fam, eta, z, lq, want, _ = _kl_case("mvn", 5, 3, 129)
    bad = eta.copy()
    bad[1, 5] = 1.0  # P_00 = -2: not positive definite
    got = host(fam.KL_device(dev(z), dev(lq), dev(bad)))
    assert np.isnan(got[1]) and np.isnan(R.kl_mvn(z, lq, bad)[1])
    assert kl_err(got[[0, 2]], want[[0, 2]]) <= KL_BAR
    bad = eta.copy()
    bad[2, 5 + 4] = -10.0  # a large off-diagonal entry: the last pivot is negative
    got = host(fam.KL_device(dev(z), dev(lq), dev(bad)))
    assert np.isnan(got[2]) and np.isfinite(got[:2]).all()
    fam, eta, z, lq, want, _ = _kl_case("dir", 5, 3, 129)
    bad = eta.copy()
    bad[0, 2] = -0.5  # a negative concentration
    got = host(fam.KL_device(dev(z), dev(lq), dev(bad)))
    assert np.isnan(got[0]) and kl_err(got[1:], want[1:]) <= KL_BAR


def test_prior_and_kl_capture_in_one_graph():
    """No host synchronisation: both device methods captured in one graph, the draw index a device word incremented
    inside it; two replays give the eager results of draws 0 and 1."""
    from torch_nf_amd import _lib
    from torch_nf_amd.exponential_families import MVN

    fam = MVN(5)
    rng = np.random.RandomState(0)
    z, lq = dev(rng.normal(0, 1, (6, 40, 5))), dev(rng.normal(0, 1, (6, 40)), np.float64)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    fam.KL_device(z, lq, fam.sample_eta_device(6, seed=SEED))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eta = fam.sample_eta_device(6, seed=SEED, t_dev=counter)
        counter.add_(1)
        kl = fam.KL_device(z, lq, eta)
    for r in range(2):
        before = [_lib.lib.tnf_efn_launch_count(w) for w in range(3)]
        graph.replay()
        torch.cuda.synchronize()
        assert [_lib.lib.tnf_efn_launch_count(w) for w in range(3)] == before  # a replay does not enter the library
        want = fam.sample_eta_device(6, seed=SEED, t=r)
        assert torch.equal(eta, want) and torch.equal(kl, fam.KL_device(z, lq, want)), r
    assert int(counter.item()) == 2


# ---- 3. train_efn ---------------------------------------------------------------------------------------------------------
def _dirichlet_cde():
    import torch_nf_amd as tnf

    torch.manual_seed(5)
    nf = tnf.NormFlow(2, True, "coupling", 1, 1, 15, support_layer=tnf.ToSimplex(2))
    return tnf.ConditionalDensityEstimator(nf, 4, [16])


@functools.lru_cache(maxsize=None)
def _dirichlet_run(use_graph, num_iters=200):
    from torch_nf_amd.efn import train_efn
    from torch_nf_amd.exponential_families import Dirichlet

    cde = _dirichlet_cde()
    torch.manual_seed(7)
    return train_efn(cde, Dirichlet(3), M=8, N=32, num_iters=num_iters, lr=1e-3, seed=3, use_graph=use_graph)


def test_train_efn_first_iteration_is_the_public_pieces():
    from torch_nf_amd.efn import train_efn
    from torch_nf_amd.exponential_families import Dirichlet, efn_loss

    fam = Dirichlet(3)
    cde = _dirichlet_cde()
    torch.manual_seed(7)
    losses, KLs = train_efn(cde, fam, M=8, N=32, num_iters=1, lr=1e-3, seed=3, use_graph=False)
    assert losses.shape == (1,) and KLs.shape == (1,)
    cde = _dirichlet_cde()  # the same initial weights
    torch.manual_seed(7)
    eta = fam.sample_eta_device(8, seed=3, t=0)
    z, log_q = cde.sample(eta, 32, freeze_bn=False)
    loss = float(efn_loss(z, log_q, eta, fam).detach())
    kl = float(fam.KL_device(z.detach(), log_q.detach(), eta).mean())
    assert abs(losses[0] - loss) <= 1e-5 and abs(KLs[0] - kl) <= 1e-5, (losses, loss, KLs, kl)
    # ... and the device KL is the host KL of the same samples
    want = float(np.mean(fam.KL(host(z), host(log_q), host(eta))))
    assert abs(kl - want) <= KL_BAR * (1.0 + abs(want))


def test_train_efn_eager_run_learns():
    losses, KLs = _dirichlet_run(False)
    assert losses.shape == (200,) and KLs.shape == (200,) and np.isfinite(losses).all() and np.isfinite(KLs).all()
    print("train_efn eager: loss first / last quarter %.4f / %.4f, KL %.4f / %.4f"
          % (losses[:50].mean(), losses[150:].mean(), KLs[:50].mean(), KLs[150:].mean()))
    assert losses[150:].mean() < losses[:50].mean()


def test_train_efn_graphed_run():
    le, ke = _dirichlet_run(False)
    lg, kg = _dirichlet_run(True)
    assert lg.shape == (200,) and kg.shape == (200,) and np.isfinite(lg).all() and np.isfinite(kg).all()
    assert np.abs(lg[:3] - le[:3]).max() <= 1e-5 and np.abs(kg[:3] - ke[:3]).max() <= 1e-5  # the eager warm-up iterations
    print("train_efn graphed: loss first / last quarter %.4f / %.4f" % (lg[:50].mean(), lg[150:].mean()))
    assert lg[150:].mean() < lg[:50].mean()


def test_train_efn_stops_before_a_non_finite_iteration():
    from torch_nf_amd.efn import train_efn
    from torch_nf_amd.exponential_families import Dirichlet

    class Poisoned(Dirichlet):
        """The prior's double: the sixth draw holds an infinite concentration, as a prior with lb = -inf would give."""
        calls = 0

        def sample_eta_device(self, N, **kw):
            eta = super().sample_eta_device(N, **kw)
            self.calls += 1
            if self.calls == 6:
                eta = eta.clone()
                eta[0, 0] = float("-inf")
            return eta

    fam = Poisoned(3)
    cde = _dirichlet_cde()
    torch.manual_seed(7)
    losses, KLs = train_efn(cde, fam, M=8, N=32, num_iters=12, lr=1e-3, seed=3, prior_kwargs=dict(lb=0.5, ub=2.0),
                            use_graph=False, check_every=4)
    assert fam.calls == 8  # looked at after iterations 4 and 8
    assert losses.shape == (5,) and KLs.shape == (5,) and np.isfinite(losses).all() and np.isfinite(KLs).all()
    want, _ = _dirichlet_run(False)
    assert np.abs(losses - want[:5]).max() <= 1e-5  # the iterations before it are the unpoisoned run's


def test_train_efn_mvn():
    import torch_nf_amd as tnf
    from torch_nf_amd.efn import train_efn

    torch.manual_seed(1)
    fam = tnf.MVN(4)
    cde = tnf.ConditionalDensityEstimator(tnf.NormFlow(4, True, "coupling", 1, 2, 15), fam.D_eta, [16])
    losses, KLs = train_efn(cde, fam, M=8, N=32, num_iters=10, lr=1e-3, seed=1)
    assert losses.shape == (10,) and KLs.shape == (10,) and np.isfinite(losses).all() and np.isfinite(KLs).all()
