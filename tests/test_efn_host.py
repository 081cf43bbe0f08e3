"""The EFN prior and KL kernels without a GPU: header, exports and binding table in step; every refusal of
include/tnf_efn.h that precedes a launch; what the wrappers of efn_ops.py hand to the library; train_efn's argument
errors and its torch_nf alias; and the float64 restatement (tests/efn_restatement.py) against the package's own
conversions and the reference's KL values of tests/golden/expfam.npz."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import efn_restatement as R

import torch_nf_amd as tnf
from torch_nf_amd import _lib, efn_ops
from torch_nf_amd.efn import train_efn
from torch_nf_amd.exponential_families import MVN, Dirichlet

INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
MVN_F, DIR_F = _lib.EF_MVN, _lib.EF_DIRICHLET


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_efn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.EFN_SIGNATURES) and len(protos) == 7
    others = set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
    assert not set(_lib.EFN_SIGNATURES) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.EFN_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t, int32_t and float
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32 \
                if "int32_t" in p else ctypes.c_float
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p or "float " in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "tnf_efn.h")).read()
    assert '#include "tnf_efn.h"' in open(os.path.join(ROOT, "include", "tnf.h")).read()
    for n in ("EFN_COUNT_PRIOR", "EFN_COUNT_NOISE", "EFN_COUNT_KL"):
        assert "TNF_%s = %d" % (n, getattr(_lib, n)) in header
    assert "TNF_EFN_COUNTERS = 3" in header
    assert "#define TNF_EFN_MAX_D %d" % _lib.EFN_MAX_D in header and _lib.EFN_MAX_D == 64
    assert "#define TNF_EFN_MAX_DF %d" % _lib.EFN_MAX_DF in header and _lib.EFN_MAX_DF == 1024
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set


def test_queries_host_side():
    lib = _lib.lib
    for fam in (MVN_F, DIR_F):
        assert [lib.tnf_efn_supported(fam, D) for D in range(0, 67)] == [0] + [1] * 64 + [0, 0]
        assert lib.tnf_efn_supported(fam, -1) == 0
    assert lib.tnf_efn_supported(2, 5) == 0 and lib.tnf_efn_supported(-1, 5) == 0
    for which in range(3):
        assert lib.tnf_efn_launch_count(which) >= 0
    assert lib.tnf_efn_launch_count(3) == -1 and b"tnf_efn_launch_count" in lib.tnf_last_error()
    assert lib.tnf_efn_launch_count(-1) == -1
    assert lib.tnf_efn_prior_num_noise(MVN_F, 5, 5) == 5 * 26 and lib.tnf_efn_prior_num_noise(MVN_F, 64, 16) == 64 * 1025
    assert lib.tnf_efn_prior_num_noise(MVN_F, 1, 1) == 2 and lib.tnf_efn_prior_num_noise(DIR_F, 7, -3) == 7
    assert lib.tnf_efn_prior_num_noise(MVN_F, 64, 17) == -1 and lib.tnf_efn_prior_num_noise(MVN_F, 5, 0) == -1
    assert lib.tnf_efn_prior_num_noise(MVN_F, 65, 1) == -1 and lib.tnf_efn_prior_num_noise(3, 5, 5) == -1
    # workspace: M * (G * 8 + (D_eta + 1) * 4), G = workgroups per context, at most 8192 / M of them and one per tile
    assert lib.tnf_efn_kl_workspace_bytes(DIR_F, 100, 100, 5) == 100 * (1 * 8 + 7 * 4)
    assert lib.tnf_efn_kl_workspace_bytes(MVN_F, 64, 1024, 64) == 64 * (8 * 8 + (64 + 2080 + 1) * 4)
    assert lib.tnf_efn_kl_workspace_bytes(MVN_F, 1, 1 << 24, 2) == 8192 * 8 + 6 * 4
    assert lib.tnf_efn_kl_workspace_bytes(MVN_F, 0, 5, 2) == 0
    for bad in ((MVN_F, 1, 0, 2), (MVN_F, -1, 5, 2), (MVN_F, 1, 5, 65), (2, 1, 5, 2), (MVN_F, 1, 5, 0)):
        assert lib.tnf_efn_kl_workspace_bytes(*bad) == -1


def test_argument_refusals_without_launching():
    lib = _lib.lib
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(6)]  # never dereferenced: every call fails validation first
    counts = [lib.tnf_efn_launch_count(w) for w in range(3)]

    def prior(**kw):
        a = dict(eta=p[0], noise=None, t_dev=None, family=MVN_F, D=5, fac=5, sigma_mu=1.0, lb=0.5, ub=2.0, seed=1, t=0, i0=0,
                 M=4)
        a.update(kw)
        return lib.tnf_efn_prior_f32(a["eta"], a["noise"], a["t_dev"], a["family"], a["D"], a["fac"], a["sigma_mu"], a["lb"],
                                     a["ub"], a["seed"], a["t"], a["i0"], a["M"], None)

    def noise(**kw):
        a = dict(noise=p[0], t_dev=None, family=MVN_F, D=5, fac=5, seed=1, t=0, i0=0, M=4)
        a.update(kw)
        return lib.tnf_efn_prior_noise_f32(a["noise"], a["t_dev"], a["family"], a["D"], a["fac"], a["seed"], a["t"], a["i0"],
                                           a["M"], None)

    def kl(**kw):
        a = dict(z=p[0], log_q=p[1], dtype=_lib.F32, eta=p[2], kl=p[3], family=MVN_F, M=3, N=7, D=5, ws=p[4], ws_bytes=1 << 20)
        a.update(kw)
        return lib.tnf_efn_kl_f32(a["z"], a["log_q"], a["dtype"], a["eta"], a["kl"], a["family"], a["M"], a["N"], a["D"],
                                  a["ws"], a["ws_bytes"], None)

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, msg)

    for fam in (MVN_F, DIR_F):
        refused(prior(family=fam, eta=None), INV, b"tnf_efn_prior_f32: NULL pointer")
        for D in (0, 65, -4):
            refused(prior(family=fam, D=D), UNSUP, b"tnf_efn_prior_f32: family=%d D=%d" % (fam, D))
            refused(noise(family=fam, D=D), UNSUP, b"tnf_efn_prior_noise_f32: family=%d D=%d" % (fam, D))
        for kw in (dict(t=-1), dict(t=1 << 31), dict(i0=-1), dict(M=-1), dict(i0=(1 << 31) - 3), dict(M=(1 << 31) + 1)):
            refused(prior(family=fam, **kw), INV, b"outside the stream's counters")
            refused(noise(family=fam, **kw), INV, b"outside the stream's counters")
    refused(prior(family=2), UNSUP, b"family=2 D=5")
    for fac in (0, -1):
        refused(prior(fac=fac), INV, b"iw_df_fac=%d, must be at least 1" % fac)
        refused(noise(fac=fac), INV, b"iw_df_fac=%d, must be at least 1" % fac)
    refused(prior(fac=205), INV, b"df=1025, the chi-square sums serve df <= 1024")
    refused(prior(D=64, fac=17), INV, b"df=1088")
    refused(noise(D=64, fac=17), INV, b"df=1088")
    refused(prior(fac=1 << 30, D=64), INV, b"the chi-square sums serve")
    refused(prior(sigma_mu=-1.0), INV, b"sigma_mu=-1, must be >= 0")
    refused(prior(sigma_mu=float("nan")), INV, b"must be >= 0")
    for lb, ub in ((2.0, 0.5), (float("-inf"), 1.0), (0.0, float("inf")), (float("nan"), 1.0), (0.0, float("nan"))):
        refused(prior(family=DIR_F, lb=lb, ub=ub), INV, b"must be finite with lb <= ub")
    assert prior(family=DIR_F, fac=0, sigma_mu=-1.0, M=0) == 0  # read for MVN only
    assert prior(lb=3.0, ub=1.0, M=0) == 0                       # read for Dirichlet only
    assert prior(M=0) == 0 and noise(M=0) == 0 and prior(family=DIR_F, M=0) == 0  # nothing to do: OK, no launch
    refused(noise(noise=None), INV, b"tnf_efn_prior_noise_f32: NULL pointer")

    for name in ("z", "log_q", "eta", "kl", "ws"):
        refused(kl(**{name: None}), INV, b"tnf_efn_kl_f32: NULL pointer")
    for D in (0, 65):
        refused(kl(D=D), UNSUP, b"tnf_efn_kl_f32: family=0 D=%d" % D)
    refused(kl(family=7), UNSUP, b"family=7")
    refused(kl(dtype=2), INV, b"log_q_dtype=2")
    refused(kl(N=0), INV, b"N=0")
    refused(kl(M=-1), INV, b"M=-1")
    need = lib.tnf_efn_kl_workspace_bytes(MVN_F, 3, 7, 5)
    refused(kl(ws_bytes=need - 1), WS, b"workspace of %d B, %d B needed" % (need - 1, need))
    assert kl(M=0, ws_bytes=0) == 0
    assert [lib.tnf_efn_launch_count(w) for w in range(3)] == counts  # nothing was launched


# ---- what the wrappers hand over -----------------------------------------------------------------------------------------
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name in ("tnf_efn_supported", "tnf_efn_prior_num_noise", "tnf_efn_kl_workspace_bytes"):
            return getattr(_lib.lib, name)

        def call(*args):
            assert len(args) == len(_lib.EFN_SIGNATURES[name][1]), name
            self.calls.append((name, args))
            return 0

        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "require_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(efn_ops, "lib", rec)
    return rec


def test_wrapper_marshalling(recorder):
    t_dev = torch.zeros(1, dtype=torch.int64)
    eta = efn_ops.efn_prior(MVN_F, 5, 7, iw_df_fac=3, sigma_mu=2.0, seed=-1, t=4, i0=9)
    assert recorder.calls[-1] == ("tnf_efn_prior_f32", (eta.data_ptr(), None, None, MVN_F, 5, 3, 2.0, 0.5, 2.0,
                                                         0x7FFFFFFFFFFFFFFF, 4, 9, 7, 0))
    assert tuple(eta.shape) == (7, 20) and eta.dtype == torch.float32
    rec = torch.zeros(7, 5)
    eta = efn_ops.efn_prior(DIR_F, 5, 7, lb=1.0, ub=3.0, seed=6, noise=rec, t_dev=t_dev)
    assert recorder.calls[-1][1] == (eta.data_ptr(), rec.data_ptr(), t_dev.data_ptr(), DIR_F, 5, 5, 1.0, 1.0, 3.0, 6, 0, 0, 7, 0)
    assert tuple(eta.shape) == (7, 6)
    nz = efn_ops.efn_prior_noise(MVN_F, 3, 2, iw_df_fac=2, seed=5, t=1, i0=8, t_dev=t_dev)
    assert recorder.calls[-1] == ("tnf_efn_prior_noise_f32", (nz.data_ptr(), t_dev.data_ptr(), MVN_F, 3, 2, 5, 1, 8, 2, 0))
    assert tuple(nz.shape) == (2, 3 * 7) and tuple(efn_ops.efn_prior_noise(DIR_F, 3, 2).shape) == (2, 3)
    calls = len(recorder.calls)
    assert tuple(efn_ops.efn_prior(MVN_F, 5, 0).shape) == (0, 20) and tuple(efn_ops.efn_prior_noise(DIR_F, 3, 0).shape) == (0, 3)
    assert len(recorder.calls) == calls  # no context: no call
    z, e = torch.zeros(3, 7, 5), torch.zeros(3, 20)
    for lq, code in ((torch.zeros(3, 7), _lib.F32), (torch.zeros(3, 7, dtype=torch.float64), _lib.F64)):
        kl = efn_ops.efn_kl(MVN_F, z, lq, e)
        name, a = recorder.calls[-1]
        assert name == "tnf_efn_kl_f32" and a[:9] == (z.data_ptr(), lq.data_ptr(), code, e.data_ptr(), kl.data_ptr(), MVN_F, 3, 7, 5)
        assert a[10] >= _lib.lib.tnf_efn_kl_workspace_bytes(MVN_F, 3, 7, 5) and a[11] == 0
        assert tuple(kl.shape) == (3,) and kl.dtype == torch.float32


def test_wrapper_refusals(recorder):
    for fam, D in ((MVN_F, 0), (MVN_F, 65), (DIR_F, 65), (2, 5), (MVN_F, 5.0)):
        with pytest.raises(ValueError, match="1 <= D <= 64"):
            efn_ops.efn_prior(fam, D, 3)
    for fac in (0, 205, 2.0):
        with pytest.raises(ValueError, match="iw_df_fac"):
            efn_ops.efn_prior(MVN_F, 5, 3, iw_df_fac=fac)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_mu"):
            efn_ops.efn_prior(MVN_F, 5, 3, sigma_mu=bad)
    for lb, ub in ((2.0, 1.0), (float("-inf"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="lb and ub"):
            efn_ops.efn_prior(DIR_F, 5, 3, lb=lb, ub=ub)
    for M in (-1, 2.0):
        with pytest.raises(ValueError, match="number of contexts"):
            efn_ops.efn_prior(DIR_F, 5, M)
    with pytest.raises(ValueError, match="noise must be float32"):
        efn_ops.efn_prior(DIR_F, 5, 3, noise=torch.zeros(3, 4))
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="t_dev must be one int64"):
            efn_ops.efn_prior(DIR_F, 5, 3, t_dev=bad)
    z, lq, e = torch.zeros(3, 7, 5), torch.zeros(3, 7), torch.zeros(3, 20)
    with pytest.raises(ValueError, match=r"z must be \(M, N, D\)"):
        efn_ops.efn_kl(MVN_F, z[0], lq, e)
    with pytest.raises(TypeError, match="float32 only"):
        efn_ops.efn_kl(MVN_F, z.double(), lq, e)
    with pytest.raises(TypeError, match="log_q must be"):
        efn_ops.efn_kl(MVN_F, z, lq.half(), e)
    for args in ((z, lq[:, :6], e), (z, lq, e[:, :19]), (z[:, :0], lq[:, :0], e)):
        with pytest.raises(ValueError, match="need N >= 1"):
            efn_ops.efn_kl(MVN_F, *args)
    with pytest.raises(ValueError, match="1 <= D <= 64"):
        efn_ops.efn_kl(DIR_F, torch.zeros(3, 7, 65), lq, torch.zeros(3, 66))
    assert not recorder.calls


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        MVN(3).sample_eta_device(4)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        Dirichlet(3).sample_eta_device(4)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        Dirichlet(3).KL_device(torch.zeros(2, 4, 3), torch.zeros(2, 4), torch.ones(2, 4))
    with pytest.raises(NotImplementedError):
        tnf.ExponentialFamily(3).sample_eta_device(4)


# ---- the restatement against the package's conversions and the reference's KL -----------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 5, 16])
@pytest.mark.parametrize("fac", [2, 5])
def test_mvn_restatement_is_mu_to_eta_of_the_inverse(D, fac):
    """The kernel's shortcut -- W is the precision, nothing is inverted -- against the reference's route: Sigma = inv(W),
    then mu_to_eta(mu, Sigma), which inverts Sigma again (pinned to the reference by tests/golden/expfam.npz)."""
    df = fac * D
    rng = np.random.RandomState(10 * D + fac)
    noise = rng.normal(0.0, 1.0, (6, R.mvn_num_noise(D, df)))
    mu, L, W = R.mvn_parts(noise, D, df, sigma_mu=1.5)
    assert np.array_equal(mu, 1.5 * noise[:, :D]) and np.array_equal(np.triu(L, 1), np.zeros_like(L))
    assert np.array_equal(L[:, 1:, 0], noise[:, [D + i * (i - 1) // 2 for i in range(1, D)]])  # row-major strict lower
    chi0 = noise[:, D + D * (D - 1) // 2:][:, :df]
    np.testing.assert_allclose(L[:, 0, 0] ** 2, np.sum(chi0 ** 2, axis=1), rtol=1e-14)
    eta = R.mvn_eta(noise, D, df, sigma_mu=1.5)
    want = MVN(D).mu_to_eta(mu, np.linalg.inv(W))
    np.testing.assert_allclose(eta, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())


def test_dirichlet_restatement_is_mu_to_eta():
    u = np.random.RandomState(3).uniform(0, 1, (6, 7))
    eta = R.dirichlet_eta(u, 0.5, 2.0)
    assert np.array_equal(eta, Dirichlet(7).mu_to_eta(0.5 + 1.5 * u)) and (eta[:, 7] == 1.0).all()


@pytest.mark.parametrize("D", [2, 5, 20])
def test_kl_restatement_reproduces_the_reference(D):
    g = load_golden("expfam")
    for name, fn in (("mvn", R.kl_mvn), ("dir", R.kl_dirichlet)):
        k = "%s%d_" % (name, D)
        got = fn(g[k + "z64"], g[k + "lp"], g[k + "eta"][:3])
        np.testing.assert_allclose(got, g[k + "KL"], rtol=1e-9, atol=0)


def test_kl_restatement_conventions():
    rng = np.random.RandomState(5)
    fam = MVN(3)
    noise = rng.normal(0, 1, (3, R.mvn_num_noise(3, 15)))
    eta = R.mvn_eta(noise, 3, 15)
    z, lq = rng.normal(0, 1, (3, 9, 3)), rng.normal(0, 1, (3, 9))
    np.testing.assert_allclose(R.kl_mvn(z, lq, eta), fam.KL(z, lq, eta), rtol=1e-10)
    eta[1, 3] = 1.0  # P_00 = -2: not positive definite
    got = R.kl_mvn(z, lq, eta)
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all()
    zd = rng.dirichlet(np.ones(4), (2, 9))
    zd[0, 0] = [0.0, 0.5, 0.5, 0.0]  # exact zeros: the 1e-32 nudge keeps log finite
    e = R.dirichlet_eta(rng.uniform(0, 1, (2, 4)), 0.5, 2.0)
    got = R.kl_dirichlet(zd, lq[:2], e)
    np.testing.assert_allclose(got, Dirichlet(4).KL(zd, lq[:2], e), rtol=1e-12)
    assert np.isfinite(got).all()
    bar = R.eta_bar(np.array([[1.0, -8.0], [0.5, 0.25]]), 2, 10)
    np.testing.assert_allclose(bar, [4 * 10 * 2.0 ** -24 * 8.0, 4 * 10 * 2.0 ** -24 * 0.5])
    assert R.eta_bar(np.array([[2.0, 1.0]]), 64, 64)[0] == 4 * 64 * 2.0 ** -24 * 2.0
    assert R.eta_bar(np.array([[2.0, 1.0]]), 1)[0] == 4 * 2.0 ** -24 * 2.0


# ---- train_efn ------------------------------------------------------------------------------------------------------------
def _dirichlet_cde(D=3, hidden=(16,)):
    nf = tnf.NormFlow(D - 1, True, "coupling", 1, 1, 15, support_layer=tnf.ToSimplex(D - 1), device="cpu")
    return tnf.ConditionalDensityEstimator(nf, D + 1, list(hidden))


def test_train_efn_argument_errors():
    fam = Dirichlet(3)
    cde = _dirichlet_cde()
    for kw in (dict(M=0), dict(M=2.0), dict(N=0), dict(N=-5), dict(num_iters=0), dict(num_iters=1.5), dict(check_every=0),
               dict(check_every=None)):
        with pytest.raises(ValueError, match="must be a positive int"):
            train_efn(cde, fam, **kw)
    with pytest.raises(ValueError, match="width 3, the family has D=4"):
        train_efn(cde, Dirichlet(4))
    with pytest.raises(ValueError, match="width 3, the family has D=2"):
        train_efn(cde, Dirichlet(2))
    nf = tnf.NormFlow(3, True, "coupling", 1, 1, 15, device="cpu")  # no support layer: width D
    with pytest.raises(ValueError, match="D_x=4, the family has D_eta=9"):
        train_efn(tnf.ConditionalDensityEstimator(nf, 4, [8]), MVN(3))
    with pytest.raises(ValueError, match="width 3, the family has D=4"):
        train_efn(tnf.ConditionalDensityEstimator(nf, 14, [8]), MVN(4))
    wide = tnf.ConditionalDensityEstimator(tnf.NormFlow(2, True, "coupling", 1, 1, 15, support_layer=tnf.ToSimplex(2),
                                                        device="cpu"), 7, [8])
    with pytest.raises(ValueError, match="D_x=7, the family has D_eta=4"):
        train_efn(wide, fam)
    with pytest.raises(ValueError, match="must draw and score on the device"):
        train_efn(cde, object())


def test_exports_and_torch_nf_alias():
    assert "train_efn" in tnf.__all__ and tnf.train_efn is train_efn
    tnf.install_as_torch_nf()
    ns = {}
    exec("from torch_nf.efn import train_efn", ns)
    assert ns["train_efn"] is train_efn
