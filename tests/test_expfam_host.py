"""Host side of torch_nf_amd.exponential_families: constructors, parameter conversions, prior draws and KL against the
reference's recorded results (tests/golden/expfam.npz, written by tools/gen_expfam_golden.py), the torch_nf alias, and
the argument checks of the tnf_ef_* entries.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

FAMS = [("mvn", "MVN"), ("dir", "Dirichlet")]
DS = [2, 5, 20]


@pytest.fixture(scope="module")
def ef():
    from torch_nf_amd import exponential_families

    return exponential_families


@pytest.fixture(scope="module")
def gold():
    return load_golden("expfam")


def test_exponential_family_init(ef):
    from torch_nf_amd.bijectors import Bijector, ToInterval, ToSimplex

    fam = ef.ExponentialFamily(4)
    assert fam.D == 4 and fam.D_eta == 4 and fam.support_layer is None
    assert ef.ExponentialFamily(3, ToInterval).support_layer is ToInterval
    assert ef.ExponentialFamily(3, Bijector).support_layer is Bijector
    for bad in ("foo", 2.0, np.int64(3), True, None):
        with pytest.raises(TypeError):
            ef.ExponentialFamily(bad)
    with pytest.raises(TypeError, match="ExponentialFamily argument D must be int not str."):
        ef.ExponentialFamily("foo")
    for bad in (0, -1):
        with pytest.raises(ValueError):
            ef.ExponentialFamily(bad)
    for bad in ("foo", 3, ToSimplex(3), int):
        with pytest.raises(TypeError):
            ef.ExponentialFamily(4, bad)
    for call in (lambda: fam.sample_eta(10), lambda: fam.mu_to_eta(None), lambda: fam.eta_to_mu(None),
                 lambda: fam.T(None)):
        with pytest.raises(NotImplementedError):
            call()


@pytest.mark.parametrize("D", [1, 2, 5, 20, 64])
def test_family_dims_and_support(ef, D):
    from torch_nf_amd.bijectors import ToSimplex

    mvn, dr = ef.MVN(D), ef.Dirichlet(D)
    assert mvn.D_eta == D + D * (D + 1) // 2 and type(mvn.D_eta) is int and mvn.support_layer is None
    assert dr.D_eta == D + 1 and dr.support_layer is ToSimplex
    with pytest.raises(TypeError):
        ef.MVN(float(D))
    with pytest.raises(ValueError):
        ef.Dirichlet(0)


@pytest.mark.parametrize("D", DS)
def test_mvn_conversions_match_reference(ef, gold, D):
    fam, k = ef.MVN(D), "mvn%d_" % D
    mu, Sigma = fam.eta_to_mu(gold[k + "eta"])
    assert mu.dtype == np.float64 and Sigma.dtype == np.float64
    assert np.allclose(mu, gold[k + "mu"]) and np.allclose(Sigma, gold[k + "Sigma"])
    eta = fam.mu_to_eta(gold[k + "mu"], gold[k + "Sigma"])
    assert eta.dtype == np.float64 and eta.shape == (5, fam.D_eta)
    assert np.allclose(eta, gold[k + "eta_rt"]) and np.allclose(eta, gold[k + "eta"])
    # mutual inverses on fresh parameters; packing order (0,0),(0,1)..(0,D-1),(1,1)..
    rng = np.random.RandomState(D)
    A = rng.normal(size=(4, D, D))
    S = np.eye(D) + np.matmul(A, A.transpose(0, 2, 1)) / 2
    m = rng.normal(size=(4, D))
    e = fam.mu_to_eta(m, S)
    m2, S2 = fam.eta_to_mu(e)
    assert np.allclose(m2, m) and np.allclose(S2, S)
    P = np.linalg.inv(S)
    r, c = np.triu_indices(D)
    assert np.allclose(e[:, :D], np.einsum("nij,nj->ni", P, m))
    assert np.allclose(e[:, D:], np.where(r == c, -0.5, -1.0) * P[:, r, c])


@pytest.mark.parametrize("D", DS)
def test_dirichlet_conversions_match_reference(ef, gold, D):
    fam, k = ef.Dirichlet(D), "dir%d_" % D
    alpha = fam.eta_to_mu(gold[k + "eta"])
    assert np.allclose(alpha, gold[k + "alpha"]) and alpha.shape == (5, D)
    eta = fam.mu_to_eta(gold[k + "alpha"])
    assert np.allclose(eta, gold[k + "eta_rt"]) and np.allclose(eta, gold[k + "eta"])
    assert np.array_equal(eta[:, D], np.ones(5))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name,cls", FAMS)
def test_KL_matches_reference(ef, gold, name, cls, D):
    import torch

    fam, k = getattr(ef, cls)(D), "%s%d_" % (name, D)
    KL = fam.KL(gold[k + "z64"], gold[k + "lp"], gold[k + "eta"][:3])
    assert KL.shape == (3,) and KL.dtype == np.float64
    np.testing.assert_allclose(KL, gold[k + "KL"], rtol=1e-9)
    # host tensors (as the training loop hands them over) give the same
    KLt = fam.KL(torch.from_numpy(gold[k + "z64"]).requires_grad_(), torch.from_numpy(gold[k + "lp"]), gold[k + "eta"][:3])
    assert np.array_equal(KLt, KL)


def test_mvn_sample_eta(ef):
    D = 4
    fam = ef.MVN(D)
    for N in (1, 50):
        np.random.seed(0)
        eta = fam.sample_eta(N)
        assert eta.shape == (N, fam.D_eta) and eta.dtype == np.float64 and np.all(np.isfinite(eta))
    assert fam.sample_eta().shape == (50, fam.D_eta)
    np.random.seed(3)
    a = fam.sample_eta(7)
    np.random.seed(3)
    assert np.array_equal(a, fam.sample_eta(7))  # np.random.seed governs the draw
    # larger sigma_mu -> larger var(mu); larger iw_df_fac -> Sigma closer to I
    var_mu, dist_I = [], []
    for sigma_mu, fac in ((0.1, 5), (1.0, 50), (10.0, 500)):
        np.random.seed(1)
        mu, Sigma = fam.eta_to_mu(fam.sample_eta(200, sigma_mu=sigma_mu, iw_df_fac=fac))
        var_mu.append(np.var(mu))
        dist_I.append(np.mean(np.square(Sigma - np.eye(D))))
        assert np.all(np.linalg.eigvalsh(Sigma) > 0)
    assert var_mu[0] < var_mu[1] < var_mu[2]
    assert dist_I[0] > dist_I[1] > dist_I[2]


def test_inverse_wishart_mean(ef):
    """Sigma ~ IW(df, psi I) with psi = df has E[Sigma_ii] = psi / (df - D - 1) and
    Var[Sigma_ii] = 2 psi^2 / ((df - D - 1)^2 (df - D - 3)): the sample mean over N draws must sit within 5 standard
    errors."""
    D, fac, N = 3, 5, 4000
    fam = ef.MVN(D)
    np.random.seed(12345)
    _, Sigma = fam.eta_to_mu(fam.sample_eta(N, iw_df_fac=fac))
    df = fac * D
    mean = df / (df - D - 1.0)
    se = np.sqrt(2.0 * df ** 2 / ((df - D - 1.0) ** 2 * (df - D - 3.0)) / N)
    diag = Sigma[:, np.arange(D), np.arange(D)]
    assert diag.shape == (N, D)
    assert np.all(np.abs(diag.mean(axis=0) - mean) < 5 * se), (diag.mean(axis=0), mean, se)
    off = Sigma[:, 0, 1]
    assert abs(off.mean()) < 5 * off.std() / np.sqrt(N)  # E[Sigma_ij] = 0 off the diagonal


def test_dirichlet_sample_eta(ef):
    fam = ef.Dirichlet(5)
    for N in (1, 50):
        eta = fam.sample_eta(N)
        assert eta.shape == (N, 6) and np.array_equal(eta[:, 5], np.ones(N))
        assert np.all(eta[:, :5] >= 0.5) and np.all(eta[:, :5] <= 2.0)
    assert fam.sample_eta().shape == (50, 6)
    widths = []
    for lb, ub in ((0.9, 1.1), (0.5, 2.0), (0.1, 10.0)):
        np.random.seed(2)
        alpha = fam.eta_to_mu(fam.sample_eta(500, lb=lb, ub=ub))
        assert alpha.min() >= lb and alpha.max() <= ub
        widths.append(alpha.max() - alpha.min())
    assert widths[0] < widths[1] < widths[2]


def test_install_as_torch_nf_aliases_exponential_families(ef):
    import torch_nf_amd

    torch_nf_amd.install_as_torch_nf()
    from torch_nf.exponential_families import MVN, Dirichlet, ExponentialFamily  # noqa: F401

    assert MVN is ef.MVN and Dirichlet is ef.Dirichlet
    assert torch_nf_amd.MVN is ef.MVN and "exponential_families" in torch_nf_amd.__all__
    assert callable(ef.efn_loss)


def test_eta_dot_T_shape_checks_before_any_device_work(ef):
    import torch

    fam = ef.MVN(3)
    z = torch.zeros(2, 4, 3)
    with pytest.raises(RuntimeError, match="batch dimensions"):
        fam.eta_dot_T(z, torch.zeros(3, fam.D_eta))
    with pytest.raises(ValueError):
        fam.eta_dot_T(z, torch.zeros(2, fam.D_eta + 1))
    with pytest.raises(ValueError):
        fam.eta_dot_T(torch.zeros(2, 4, 5), torch.zeros(2, fam.D_eta))
    with pytest.raises(NotImplementedError):
        ef.ExponentialFamily(3).eta_dot_T(z, torch.zeros(2, 3))


def test_cabi_host_side():
    from torch_nf_amd import _lib

    lib = _lib.lib
    for D in (1, 2, 5, 20, 64, 100):
        assert lib.tnf_ef_num_eta(_lib.EF_MVN, D) == D + D * (D + 1) // 2
        assert lib.tnf_ef_num_eta(_lib.EF_DIRICHLET, D) == D + 1
    assert lib.tnf_ef_num_eta(2, 4) == -1 and b"family" in lib.tnf_last_error()
    assert lib.tnf_ef_num_eta(_lib.EF_MVN, 0) == -1
    for fam in (_lib.EF_MVN, _lib.EF_DIRICHLET):
        assert all(lib.tnf_ef_dot_supported(fam, D) == 1 for D in range(1, 65))
        assert lib.tnf_ef_dot_supported(fam, 65) == 0 and lib.tnf_ef_dot_supported(fam, 0) == 0
    assert lib.tnf_ef_dot_supported(7, 8) == 0
    assert (_lib.EF_COUNT_DOT, _lib.EF_COUNT_DOT_BWD) == (0, 1) and lib.tnf_ef_launch_count(2) == -1
    assert lib.tnf_ef_launch_count(-1) == -1 and b"counter" in lib.tnf_last_error()
    assert lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT) >= 0 and lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT_BWD) >= 0

    dummy = ctypes.c_void_p(256)  # never dereferenced: every call below fails validation first
    before = lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT), lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT_BWD)
    MVN, F32 = _lib.EF_MVN, _lib.F32
    rc = lib.tnf_ef_suffstats(F32, 5, dummy, dummy, 10, 4, None)
    assert rc == -1 and b"family" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats(9, MVN, dummy, dummy, 10, 4, None)
    assert rc == -1 and b"dtype" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats(F32, MVN, dummy, None, 10, 4, None)
    assert rc == -1 and b"NULL" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats(F32, MVN, dummy, dummy, 10, 0, None)
    assert rc == -1 and b"D=0" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats(F32, MVN, dummy, dummy, 10, 1 << 20, None)
    assert rc == _lib.EUNSUPPORTED and b"exceeds" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats_backward(_lib.F64, _lib.EF_DIRICHLET, dummy, None, dummy, 10, 4, None)
    assert rc == -1 and b"NULL" in lib.tnf_last_error()
    rc = lib.tnf_ef_suffstats_backward(F32, -1, dummy, dummy, dummy, 10, 4, None)
    assert rc == -1 and b"family" in lib.tnf_last_error()

    rc = lib.tnf_ef_dot(F32, 3, dummy, dummy, dummy, 2, 8, 4, 14, None)
    assert rc == -1 and b"family" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot(2, MVN, dummy, dummy, dummy, 2, 8, 4, 14, None)
    assert rc == -1 and b"dtype" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot(F32, MVN, dummy, None, dummy, 2, 8, 4, 14, None)
    assert rc == -1 and b"NULL" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot(F32, MVN, dummy, dummy, dummy, 2, 8, 4, 13, None)
    assert rc == -1 and b"ld_eta" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot(F32, MVN, dummy, dummy, dummy, -2, 8, 4, 14, None)
    assert rc == -1 and b"batch sizes" in lib.tnf_last_error()

    need = lib.tnf_ef_dot_bwd_workspace_bytes(MVN, 2, 1000, 4)
    assert need == 2 * 16 * 14 * 8  # 16 tiles of 64 samples per context, one partial row each
    assert lib.tnf_ef_dot_bwd_workspace_bytes(MVN, 1, 1 << 19, 64) == 256 * 2144 * 8  # 2.2 MB
    assert lib.tnf_ef_dot_bwd_workspace_bytes(MVN, 1024, 1024, 20) == 1024 * 230 * 8
    assert lib.tnf_ef_dot_bwd_workspace_bytes(4, 2, 1000, 4) == -1
    rc = lib.tnf_ef_dot_backward(F32, MVN, dummy, dummy, dummy, dummy, dummy, 2, 1000, 4, 14, dummy, need - 1, None)
    assert rc == -4 and b"workspace" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot_backward(F32, MVN, dummy, dummy, dummy, dummy, dummy, 2, 1000, 4, 14, None, need, None)
    assert rc == -4 and b"workspace" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot_backward(F32, MVN, dummy, dummy, None, dummy, dummy, 2, 1000, 4, 14, dummy, need, None)
    assert rc == -1 and b"NULL" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot_backward(F32, 2, dummy, dummy, dummy, dummy, dummy, 2, 1000, 4, 14, dummy, need, None)
    assert rc == -1 and b"family" in lib.tnf_last_error()
    rc = lib.tnf_ef_dot_backward(5, MVN, dummy, dummy, dummy, dummy, dummy, 2, 1000, 4, 14, dummy, need, None)
    assert rc == -1 and b"dtype" in lib.tnf_last_error()
    after = lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT), lib.tnf_ef_launch_count(_lib.EF_COUNT_DOT_BWD)
    assert after == before  # nothing was launched
