"""Rejection ABC without a GPU: header, exports and binding table in step; every refusal of include/tnf_abc.h that
precedes a launch; GaussianProposal, Mat.prior, Mat.abc_accept and the drivers' argument errors on the host; what the
wrappers of abc_ops.py hand to the library; the restated Philox4x32-10 against its published vectors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import abc_restatement as R

import torch_nf_amd as tnf
from torch_nf_amd import _lib, abc_ops
from torch_nf_amd.lfi import ABC_MCMC, ABC_SMC
from torch_nf_amd.systems import GaussianProposal, Mat

INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_abc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.ABC_SIGNATURES) and len(protos) == 5
    assert not set(_lib.ABC_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.ABC_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # only void*, int64_t and int32_t arguments
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "tnf_abc.h")).read()
    assert '#include "tnf_abc.h"' in open(os.path.join(ROOT, "include", "tnf.h")).read()
    for n in ("ABC_COUNT_SMC", "ABC_COUNT_PROPOSE", "ABC_COUNT_NOISE"):
        assert "TNF_%s = %d" % (n, getattr(_lib, n)) in header
    for n in ("ABC_MAX_D", "ABC_MAX_SMC_D", "ABC_MAX_TRIALS"):
        assert "#define TNF_%s %d" % (n, getattr(_lib, n)) in header


def test_queries_host_side():
    lib = _lib.lib
    assert [lib.tnf_abc_supported(d) for d in range(0, 9)] == [0, 0, 1, 1, 1, 1, 1, 0, 0]
    for which in range(3):
        assert lib.tnf_abc_launch_count(which) >= 0
    assert lib.tnf_abc_launch_count(3) == -1 and b"tnf_abc_launch_count" in lib.tnf_last_error()
    assert lib.tnf_abc_launch_count(-1) == -1


def test_argument_refusals_without_launching():
    lib = _lib.lib
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]  # never dereferenced: every call fails validation first
    counts = [lib.tnf_abc_launch_count(w) for w in range(3)]

    def smc(**kw):
        a = dict(z0=p[0], chol=p[1], bounds=p[2], x0=p[3], eps=p[4], omega=None, zs=p[5], xs=p[6], trials=p[7], seed=1, N=5,
                 T=3, d=3, mt=100)
        a.update(kw)
        return lib.tnf_abc_smc_mat_f32(a["z0"], a["chol"], a["bounds"], a["x0"], a["eps"], a["omega"], a["zs"], a["xs"],
                                       a["trials"], a["seed"], a["N"], a["T"], a["d"], a["mt"], None)

    def prop(**kw):
        a = dict(mu=p[0], chol=p[1], bounds=p[2], omega=None, z=p[3], trials=p[4], seed=1, M=5, Mmu=1, D=4, mt=100)
        a.update(kw)
        return lib.tnf_abc_propose_f32(a["mu"], a["chol"], a["bounds"], a["omega"], a["z"], a["trials"], a["seed"], a["M"],
                                       a["Mmu"], a["D"], a["mt"], None)

    def noise(**kw):
        a = dict(omega=p[0], seed=1, t=0, i0=0, n_i=4, j0=0, n_j=4, D=3)
        a.update(kw)
        return lib.tnf_abc_noise_f32(a["omega"], a["seed"], a["t"], a["i0"], a["n_i"], a["j0"], a["n_j"], a["D"], None)

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, msg)

    for name in ("z0", "chol", "bounds", "x0", "eps", "zs", "xs", "trials"):
        refused(smc(**{name: None}), INV, b"tnf_abc_smc_mat_f32: NULL pointer")
    for d in (1, 7, 0, -3):
        refused(smc(d=d), UNSUP, b"tnf_abc_smc_mat_f32: d=%d, the kernel exists for 2 <= d <= 6" % d)
    refused(smc(mt=0), INV, b"max_trials=0, must be 1 .. 16777216")
    refused(smc(mt=(1 << 24) + 1), INV, b"max_trials=16777217")
    refused(smc(N=1 << 24), INV, b"16777216 chains, the limit is 2^24 - 1")
    refused(smc(N=-1), INV, b"-1 chains")
    refused(smc(T=1 << 31), INV, b"T=2147483648 rounds")
    refused(smc(T=-1), INV, b"rounds")
    assert smc(N=0) == 0 and smc(T=0) == 0  # nothing to do: OK without a launch
    for name in ("mu", "chol", "bounds", "z", "trials"):
        refused(prop(**{name: None}), INV, b"tnf_abc_propose_f32: NULL pointer")
    for D in (0, 22):
        refused(prop(D=D), UNSUP, b"tnf_abc_propose_f32: D=%d, the kernel exists for 1 <= D <= 21" % D)
    refused(prop(mt=0), INV, b"max_trials=0")
    refused(prop(mt=(1 << 24) + 1), INV, b"max_trials=16777217")
    for Mmu in (0, 2, 4, 6):
        refused(prop(Mmu=Mmu), INV, b"M_mu=%d must be 1 or M=5" % Mmu)
    refused(prop(M=1 << 24, Mmu=1), INV, b"the limit is 2^24 - 1")
    assert prop(M=0, Mmu=0) == 0 and prop(M=0, Mmu=1) == 0
    refused(noise(omega=None), INV, b"tnf_abc_noise_f32: NULL pointer")
    for D in (0, 22):
        refused(noise(D=D), UNSUP, b"tnf_abc_noise_f32: D=%d" % D)
    for kw in (dict(t=-1), dict(t=1 << 31), dict(i0=-1), dict(n_i=-1), dict(i0=(1 << 24) - 3), dict(j0=(1 << 24) - 3),
               dict(n_j=(1 << 24) + 1), dict(j0=-2)):
        refused(noise(**kw), INV, b"outside the stream's counters")
    assert noise(n_i=0) == 0 and noise(n_j=0) == 0
    assert [lib.tnf_abc_launch_count(w) for w in range(3)] == counts  # nothing was launched


# ---- what the wrappers hand over -----------------------------------------------------------------------------------------
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "tnf_abc_supported":
            return getattr(_lib.lib, name)

        def call(*args):
            assert len(args) == len(_lib.ABC_SIGNATURES[name][1]), name
            self.calls.append((name, args))
            return 0

        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "require_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(abc_ops, "lib", rec)
    return rec


def test_wrapper_marshalling(recorder):
    d, D, N, T, mt = 3, 6, 5, 4, 32
    z0, chol, bounds = torch.zeros(N, D), torch.eye(D), torch.stack((-torch.ones(D), torch.ones(D)))
    x0, eps, omega = torch.zeros(2), torch.ones(T, 2), torch.zeros(T, N, mt, D)
    zs, xs, trials = abc_ops.abc_smc_mat(z0, chol, bounds, x0, eps, d, mt, seed=-1)
    name, a = recorder.calls[-1]
    assert name == "tnf_abc_smc_mat_f32" and a[:5] == tuple(t.data_ptr() for t in (z0, chol, bounds, x0, eps))
    assert a[5] is None and a[6:9] == (zs.data_ptr(), xs.data_ptr(), trials.data_ptr())
    assert a[9:] == (0x7FFFFFFFFFFFFFFF, N, T, d, mt, 0)
    assert tuple(zs.shape) == (T, N, D) and tuple(xs.shape) == (T, N, 2) and tuple(trials.shape) == (T, N)
    assert zs.dtype == xs.dtype == torch.float32 and trials.dtype == torch.int32
    abc_ops.abc_smc_mat(z0, chol, bounds, x0, eps, d, mt, 7, omega)
    assert recorder.calls[-1][1][5] == omega.data_ptr() and recorder.calls[-1][1][9] == 7
    n = len(recorder.calls)
    assert tuple(abc_ops.abc_smc_mat(z0[:0], chol, bounds, x0, eps, d, mt)[0].shape) == (T, 0, D) and len(recorder.calls) == n
    z, tr = abc_ops.abc_propose(torch.zeros(1, D), chol, bounds, 9, mt, 3)
    name, a = recorder.calls[-1]
    assert name == "tnf_abc_propose_f32" and a[3] is None and a[4:6] == (z.data_ptr(), tr.data_ptr())
    assert a[6:] == (3, 9, 1, D, mt, 0) and tuple(z.shape) == (9, D) and tr.dtype == torch.int32
    abc_ops.abc_propose(torch.zeros(9, D), chol, bounds, 9, mt, 3, torch.zeros(9, mt, D))
    assert recorder.calls[-1][1][6:] == (3, 9, 9, D, mt, 0) and recorder.calls[-1][1][3] is not None
    om = abc_ops.abc_noise(5, 2, 3, 4, 6, 7, D)
    assert recorder.calls[-1] == ("tnf_abc_noise_f32", (om.data_ptr(), 5, 2, 3, 4, 6, 7, D, 0))
    assert tuple(om.shape) == (4, 7, D) and om.dtype == torch.float32
    n = len(recorder.calls)
    assert tuple(abc_ops.abc_noise(5, 2, 3, 0, 6, 7, D).shape) == (0, 7, D) and len(recorder.calls) == n  # nothing to write


def test_wrapper_refusals(recorder):
    D, mt = 6, 32
    z0, chol, bounds = torch.zeros(5, D), torch.eye(D), torch.zeros(2, D)
    x0, eps = torch.zeros(2), torch.ones(4, 2)
    for d in (1, 7, 3.0):
        with pytest.raises(ValueError, match="2 <= d <= 6"):
            abc_ops.abc_smc_mat(z0, chol, bounds, x0, eps, d, mt)
    for bad in (0, (1 << 24) + 1, 10.0):
        with pytest.raises(ValueError, match="max_trials"):
            abc_ops.abc_smc_mat(z0, chol, bounds, x0, eps, 3, bad)
    with pytest.raises(TypeError, match="float32 only"):
        abc_ops.abc_smc_mat(z0.double(), chol, bounds, x0, eps, 3, mt)
    with pytest.raises(ValueError, match=r"z0 must be \(N, D=6\)"):
        abc_ops.abc_smc_mat(torch.zeros(5, 5), chol, bounds, x0, eps, 3, mt)
    with pytest.raises(ValueError, match="eps must be"):
        abc_ops.abc_smc_mat(z0, chol, bounds, x0, torch.ones(4, 3), 3, mt)
    with pytest.raises(ValueError, match="chol must be"):
        abc_ops.abc_smc_mat(z0, torch.eye(5), bounds, x0, eps, 3, mt)
    with pytest.raises(ValueError, match="omega must be"):
        abc_ops.abc_smc_mat(z0, chol, bounds, x0, eps, 3, mt, 0, torch.zeros(4, 5, mt + 1, D))
    with pytest.raises(ValueError, match="mu must be"):
        abc_ops.abc_propose(torch.zeros(2, D), chol, bounds, 9, mt)
    with pytest.raises(ValueError, match="mu must be"):
        abc_ops.abc_propose(torch.zeros(1, 22), torch.eye(22), torch.zeros(2, 22), 9, mt)
    with pytest.raises(ValueError, match="bounds must be"):
        abc_ops.abc_propose(torch.zeros(1, D), chol, torch.zeros(2, D + 1), 9, mt)
    assert not recorder.calls


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    mat = Mat(2)
    prop = GaussianProposal(0.25 * np.eye(3), mat.lb, mat.ub)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        prop.rvs(np.zeros(3))
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        ABC_SMC(4, mat, prop, np.array([[0.0, 1.0]]), np.ones((2, 2)))
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        ABC_MCMC(4, mat, prop, np.array([[0.0, 1.0]]), [1.0, 1.0])


# ---- systems --------------------------------------------------------------------------------------------------------------
def test_gaussian_proposal_host_side():
    rng = np.random.RandomState(0)
    D = 4
    B = rng.normal(0, 1, (D, D))
    Sigma = B @ B.T + 0.5 * np.eye(D)
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    prop = GaussianProposal(Sigma, lb, ub)
    assert prop.D == D and prop.Sigma is not None and np.array_equal(prop.lb, lb) and np.array_equal(prop.ub, ub)
    assert np.allclose(prop.L @ prop.L.T, Sigma, atol=1e-12) and np.allclose(prop.L, np.tril(prop.L))
    z, mu = rng.normal(0, 1, (7, D)), rng.normal(0, 1, D)
    diff = z - mu
    want = -0.5 * (np.einsum("ni,ij,nj->n", diff, np.linalg.inv(Sigma), diff) + np.log(np.linalg.det(Sigma))
                   + D * np.log(2 * np.pi))
    np.testing.assert_allclose(prop.logpdf(z, mu), want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(prop.pdf(z, mu), np.exp(want), rtol=1e-12)
    one = prop.logpdf(z[:1], mu)  # the notebook's call: z (1, D), mu (D) -> a scalar
    assert np.ndim(one) == 0 and abs(one - want[0]) < 1e-12
    assert np.ndim(prop.logpdf(z[0], mu)) == 0 and prop.logpdf(z, mu).shape == (7,)
    assert abs(prop.logpdf(z[0], mu) - prop.logpdf(mu, z[0])) < 1e-12  # symmetric: ABC_MCMC's ratio is degenerate
    try:
        import scipy.stats
    except ImportError:
        scipy = None
    if scipy is not None:
        dist = scipy.stats.multivariate_normal(mean=mu, cov=Sigma)
        np.testing.assert_allclose(prop.logpdf(z, mu), dist.logpdf(z), rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(prop.pdf(z, mu), dist.pdf(z), rtol=1e-10)
    with pytest.raises(ValueError, match="Sigma must be"):
        GaussianProposal(np.eye(3), lb, ub)
    with pytest.raises(ValueError, match="one length"):
        GaussianProposal(Sigma, lb, ub[:3])
    with pytest.raises(ValueError, match="lb < ub"):
        GaussianProposal(Sigma, ub, lb)
    with pytest.raises(np.linalg.LinAlgError):
        GaussianProposal(-np.eye(D), lb, ub)
    with pytest.raises(ValueError, match="must end in D=4"):
        prop.logpdf(np.zeros(3), mu)
    with pytest.raises(ValueError, match=r"mu must be \(D,\) or \(1, D\)"):
        prop.rvs(np.zeros((2, D)))
    with pytest.raises(ValueError, match="positive int"):
        prop.rvs(np.zeros(D), 0)
    big = GaussianProposal(np.eye(22), -np.ones(22), np.ones(22))
    with pytest.raises(ValueError, match="D <= 21"):
        big.rvs(np.zeros(22))


def test_mat_prior_and_abc_accept():
    mat = Mat(3)
    np.random.seed(3)
    z = mat.prior.rvs(11)
    np.random.seed(3)
    assert z.shape == (11, 6) and np.array_equal(z, mat.sample_prior(11))
    assert np.array_equal(mat.prior.logpdf(z), mat.log_prior(z)) and np.all(np.isfinite(mat.prior.logpdf(z)))
    assert mat.prior.logpdf(3.0 * np.ones(6)) == -np.inf
    x0 = np.array([[0.0, 1.5]])
    assert bool(mat.abc_accept(np.array([[0.4, 1.0]]), x0, [0.5, 0.6]))
    assert not bool(mat.abc_accept(np.array([[0.5, 1.0]]), x0, [0.5, 0.6]))  # strict
    assert not bool(mat.abc_accept(np.array([[0.4, 0.9]]), x0, [0.5, 0.6]))  # strict, every statistic
    assert not bool(mat.abc_accept(np.array([[np.nan, 1.0]]), x0, [0.5, 0.6]))
    got = mat.abc_accept(np.array([[0.4, 1.0], [0.6, 1.0], [-0.4, 2.0]]), x0, np.array([0.5, 0.6]))
    assert got.tolist() == [True, False, True]
    with pytest.raises(ValueError, match="one entry per statistic"):
        mat.abc_accept(np.zeros((1, 2)), x0, 0.5)


def test_driver_argument_errors():
    mat = Mat(2)
    prop = GaussianProposal(0.25 * np.eye(3), mat.lb, mat.ub)
    x0, eps = np.array([[0.0, 1.0]]), np.ones((3, 2))

    class Sub(Mat):
        pass

    class Other(object):
        D, D_x, d, noise = 3, 2, 2, 0.0

    for system in (Sub(2), Other()):
        with pytest.raises(ValueError, match="systems.Mat only"):
            ABC_SMC(4, system, prop, x0, eps)
    with pytest.raises(ValueError, match="noise must be 0"):
        ABC_SMC(4, Mat(2, noise=0.1), prop, x0, eps)
    m7 = Mat(7)
    with pytest.raises(ValueError, match="2 <= d <= 6"):
        ABC_SMC(4, m7, GaussianProposal(np.eye(28), m7.lb, m7.ub), x0, eps)
    m1 = Mat(1)
    with pytest.raises(ValueError, match="2 <= d <= 6"):
        ABC_SMC(4, m1, GaussianProposal(np.eye(1), m1.lb, m1.ub), x0, eps)
    with pytest.raises(ValueError, match="GaussianProposal over the system's D=3"):
        ABC_SMC(4, mat, GaussianProposal(np.eye(6), Mat(3).lb, Mat(3).ub), x0, eps)
    with pytest.raises(ValueError, match="max_trials"):
        ABC_SMC(4, mat, prop, x0, eps, max_trials=(1 << 24) + 1)
    with pytest.raises(ValueError, match="T_x0 must hold 2 statistics"):
        ABC_SMC(4, mat, prop, x0, np.ones((3, 3)))
    with pytest.raises(ValueError, match="positive int"):
        ABC_SMC(0, mat, prop, x0, eps)
    with pytest.raises(ValueError, match="positive ints"):
        ABC_MCMC(4, mat, prop, x0, [1.0, 1.0], chains=0)
    with pytest.raises(ValueError, match="systems.Mat only"):
        ABC_MCMC(4, Sub(2), prop, x0, [1.0, 1.0])
    assert "identically 0" in ABC_MCMC.__doc__


def test_exports_and_torch_nf_aliases():
    for name in ("ABC_SMC", "ABC_MCMC", "GaussianProposal", "Mat"):
        assert name in tnf.__all__ and hasattr(tnf, name)
    tnf.install_as_torch_nf()
    ns = {}
    exec("from torch_nf.systems import Mat, GaussianProposal\nfrom torch_nf.lfi import ABC_SMC", ns)
    assert ns["Mat"] is Mat and ns["GaussianProposal"] is GaussianProposal and ns["ABC_SMC"] is ABC_SMC


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_restated_philox_known_answers():
    """Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors), quoted from memory: a mismatch
    would be a reason to look again at both sides.  No independent Philox4x32 is importable here (numpy's Philox is the
    4x64 variant), so these vectors and the algebra of the paper are the check."""
    hexes = lambda w: ["%08x" % int(v) for v in w]
    assert hexes(R.philox4x32(0, 0, 0, 0, 0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert hexes(R.philox4x32(f, f, f, f, f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(R.philox4x32(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    w = R.philox4x32(np.arange(5), 2, np.arange(3)[:, None], 1, 9, 8)  # broadcasting: one block per (i, j)
    assert w[0].shape == (3, 5) and w[0].dtype == np.uint32
    assert [int(v[2, 4]) for v in w] == [int(v) for v in R.philox4x32(4, 2, 2, 1, 9, 8)]


def test_restated_stream_layout_and_twin():
    seed = (7 << 32) | 5
    om = R.noise_block(seed, 3, 2, 4, 10, 6, 7)
    assert om.shape == (4, 6, 7) and om.dtype == np.float64
    w = R.philox4x32(12, 3, 4, 1, 5, 7)  # trial j = 12 of chain i = 4 in round 3, block 1: key = (low, high) of the seed
    u1, u2 = ((int(w[0]) >> 8) + 0.5) * 2.0 ** -24, (int(w[1]) >> 8) * 2.0 ** -24
    assert abs(om[2, 2, 4] - np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)) < 1e-14
    assert abs(om[2, 2, 5] - np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2)) < 1e-14
    assert np.array_equal(R.noise_block(seed, 3, 3, 2, 12, 3, 7), om[1:3, 2:5])  # a pure function of (seed, t, i, j, k)
    assert np.array_equal(R.noise_block(seed, 3, 2, 4, 10, 6, 5), om[..., :5])
    big = R.noise_block(seed, 0, 0, 64, 0, 256, 8)
    twin = R.noise_block(seed, 0, 0, 64, 0, 256, 8, np.float32)
    assert twin.dtype == np.float32 and R.rel_err(twin, big) < 1e-4 and np.isfinite(big).all()
    assert abs(big.mean()) < 5 / np.sqrt(big.size) and abs(big.var() - 1) < 5 * np.sqrt(2 / big.size)


def test_restated_statistics_and_chain():
    rng = np.random.RandomState(1)
    for d in (2, 3, 4, 5, 6):
        mat = Mat(d)
        z = mat.sample_prior(200) if d > 2 else rng.uniform(-2, 2, (200, 3))
        want = mat.simulate(z)
        np.testing.assert_allclose(R.stats(z, d), want, rtol=1e-12, atol=1e-12)
        assert np.array_equal(R.matrices(z, d), mat.matrices(z))
        assert R.rel_err(R.stats(z, d, np.float32), want) < 1e-5
    assert R.stats(np.zeros((1, 6)), 3, np.float32).tolist() == [[0.0, 0.0]]  # a zero pivot: det 0, no NaN
    # the chain consumes the stream it restates: feeding the restated noise or naming the seed is the same thing
    d, N, T, mt, seed = 2, 6, 3, 64, 11
    z0 = np.zeros((N, 3)) + np.array([1.0, 0.0, 0.0])
    L, lb, ub, x0, eps = 0.5 * np.eye(3), -2 * np.ones(3), 2 * np.ones(3), np.array([0.0, 1.0]), np.ones((T, 2))
    omega = np.stack([R.noise_block(seed, t, 0, N, 0, mt, 3) for t in range(T)])
    a = R.smc_chain(z0, L, lb, ub, x0, eps, d, mt, omega=omega)
    b = R.smc_chain(z0, L, lb, ub, x0, eps, d, mt, seed=seed)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and (a[2] > 0).all()
    for t in range(T):
        assert np.all(np.abs(a[1][t] - x0) < eps[t]) and np.allclose(R.stats(a[0][t], d), a[1][t])
    eps[1] = 0.0
    zs, xs, trials = R.smc_chain(z0, L, lb, ub, x0, eps, d, mt, seed=seed)
    assert (trials[0] > 0).all() and (trials[1:] == 0).all() and np.isnan(zs[1:]).all() and np.isnan(xs[1:]).all()
