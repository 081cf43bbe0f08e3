"""The Hebbian learning-rule simulator without a GPU: header, exports and binding table in step; every refusal of
include/tnf_hebb.h that precedes a launch; systems.HebbLearn's constructor, bounds and prior; train_nde's argument
errors; what the wrappers of hebb_ops.py hand to the library; and the numpy restatement (tests/hebb_restatement.py)
against tests/golden/hebb.npz, the outputs of the reference notebook's own `hebb` (tools/gen_hebb_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import hebb_restatement as H

import torch_nf_amd as tnf
from torch_nf_amd import _lib, hebb_ops
from torch_nf_amd.lfi import train_nde
from torch_nf_amd.systems import HebbLearn

INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_hebb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.HEBB_SIGNATURES) and len(protos) == 4
    assert not set(_lib.HEBB_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.HEBB_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t, int32_t and one float
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32 \
                if "int32_t" in p else ctypes.c_float
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p or "float " in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "tnf_hebb.h")).read()
    assert '#include "tnf_hebb.h"' in open(os.path.join(ROOT, "include", "tnf.h")).read()
    for n in ("HEBB_COUNT_SIM", "HEBB_COUNT_NOISE"):
        assert "TNF_%s = %d" % (n, getattr(_lib, n)) in header
    assert "TNF_HEBB_COUNTERS = 2" in header
    assert "#define TNF_HEBB_MAX_N %d" % _lib.HEBB_MAX_N in header and _lib.HEBB_MAX_N == 64


def test_queries_host_side():
    lib = _lib.lib
    assert [lib.tnf_hebb_supported(n) for n in range(0, 67)] == [0] + [1] * 64 + [0, 0]
    assert lib.tnf_hebb_supported(-1) == 0
    for which in range(2):
        assert lib.tnf_hebb_launch_count(which) >= 0
    assert lib.tnf_hebb_launch_count(2) == -1 and b"tnf_hebb_launch_count" in lib.tnf_last_error()
    assert lib.tnf_hebb_launch_count(-1) == -1


def test_argument_refusals_without_launching():
    lib = _lib.lib
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]  # never dereferenced: every call fails validation first
    counts = [lib.tnf_hebb_launch_count(w) for w in range(2)]

    def sim(**kw):
        a = dict(z=p[0], x=p[1], w0=p[2], eps=None, w=p[3], traj=None, t_dev=None, seed=1, t=0, i0=0, N=5, N_w0=1, n=20,
                 N_x=50, j0=0, n_steps=100, sigma=1e-4)
        a.update(kw)
        return lib.tnf_hebb_simulate_f32(a["z"], a["x"], a["w0"], a["eps"], a["w"], a["traj"], a["t_dev"], a["seed"], a["t"],
                                         a["i0"], a["N"], a["N_w0"], a["n"], a["N_x"], a["j0"], a["n_steps"], a["sigma"], None)

    def noise(**kw):
        a = dict(omega=p[0], t_dev=None, seed=1, t=0, i0=0, n_i=4, j0=0, n_j=4, n=3)
        a.update(kw)
        return lib.tnf_hebb_noise_f32(a["omega"], a["t_dev"], a["seed"], a["t"], a["i0"], a["n_i"], a["j0"], a["n_j"], a["n"],
                                      None)

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, msg)

    for name in ("z", "x", "w0", "w"):
        refused(sim(**{name: None}), INV, b"tnf_hebb_simulate_f32: NULL pointer")
    for n in (0, 65, -4, 1000):
        refused(sim(n=n), UNSUP, b"tnf_hebb_simulate_f32: n=%d, the kernel exists for 1 <= n <= 64" % n)
    for N_w0 in (0, 2, 4, 6):
        refused(sim(N_w0=N_w0), INV, b"N_w0=%d must be 1 or N=5" % N_w0)
    refused(sim(N_x=0), INV, b"N_x=0, must be at least 1")
    refused(sim(N_x=-3), INV, b"N_x=-3")
    refused(sim(sigma=-1e-4), INV, b"sigma_eps=-0.0001, must be >= 0")
    refused(sim(sigma=float("nan")), INV, b"must be >= 0")
    for kw in (dict(t=-1), dict(t=1 << 31), dict(i0=-1), dict(N=-1), dict(i0=(1 << 31) - 4), dict(N=(1 << 31) + 1, N_w0=1),
               dict(j0=-2), dict(n_steps=-1), dict(j0=(1 << 31) - 100), dict(n_steps=1 << 31), dict(j0=1 << 31)):
        refused(sim(**kw), INV, b"outside the stream's counters")
    assert sim(N=0, N_w0=0) == 0 and sim(N=0, N_w0=1) == 0 and sim(n_steps=0) == 0  # nothing to do: OK, no launch
    assert sim(n_steps=0, N_w0=5) == 0 and sim(N=0, N_w0=0, n_steps=0, sigma=0.0) == 0
    refused(noise(omega=None), INV, b"tnf_hebb_noise_f32: NULL pointer")
    for n in (0, 65):
        refused(noise(n=n), UNSUP, b"tnf_hebb_noise_f32: n=%d" % n)
    for kw in (dict(t=-1), dict(t=1 << 31), dict(i0=-1), dict(n_i=-1), dict(i0=(1 << 31) - 3), dict(j0=(1 << 31) - 4),
               dict(n_j=1 << 31), dict(j0=-2)):
        refused(noise(**kw), INV, b"outside the stream's counters")
    assert noise(n_i=0) == 0 and noise(n_j=0) == 0
    assert [lib.tnf_hebb_launch_count(w) for w in range(2)] == counts  # nothing was launched


# ---- what the wrappers hand over -----------------------------------------------------------------------------------------
class _Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == "tnf_hebb_supported":
            return getattr(_lib.lib, name)

        def call(*args):
            assert len(args) == len(_lib.HEBB_SIGNATURES[name][1]), name
            self.calls.append((name, args))
            return 0

        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "require_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(hebb_ops, "lib", rec)
    return rec


def test_wrapper_marshalling(recorder):
    N, n, N_x, steps = 5, 20, 7, 9
    z, x, w0 = torch.zeros(N, 4), torch.zeros(N_x, n), torch.zeros(n)
    w = hebb_ops.hebb_simulate(z, x, w0, steps, 1e-4, seed=-1, t=3, i0=11, j0=2)
    name, a = recorder.calls[-1]
    assert name == "tnf_hebb_simulate_f32" and a[:2] == (z.data_ptr(), x.data_ptr()) and a[2] == w0.data_ptr()
    assert a[3] is None and a[4] == w.data_ptr() and a[5] is None and a[6] is None
    assert a[7:] == (0x7FFFFFFFFFFFFFFF, 3, 11, N, 1, n, N_x, 2, steps, 1e-4, 0)  # a (n,) start is N_w0 = 1
    assert tuple(w.shape) == (N, n) and w.dtype == torch.float32
    eps, t_dev, rows = torch.zeros(steps, N, n), torch.zeros(1, dtype=torch.int64), torch.zeros(N, n)
    w, tr = hebb_ops.hebb_simulate(z, x, rows, steps, 0.0, 7, eps=eps, traj=True, t_dev=t_dev)
    a = recorder.calls[-1][1]
    assert a[2] == rows.data_ptr() and a[3] == eps.data_ptr() and a[5] == tr.data_ptr() and a[6] == t_dev.data_ptr()
    assert a[7:] == (7, 0, 0, N, N, n, N_x, 0, steps, 0.0, 0) and tuple(tr.shape) == (steps, N, n)
    assert hebb_ops.hebb_simulate(z, x, torch.zeros(1, n), steps, 0.0) is not None and recorder.calls[-1][1][11] == 1
    calls = len(recorder.calls)
    start = torch.arange(n, dtype=torch.float32)
    assert torch.equal(hebb_ops.hebb_simulate(z, x, start, 0, 1e-4), start.expand(N, n))  # no step: the w0 rows, no call
    w, tr = hebb_ops.hebb_simulate(z[:0], x, start, steps, 1e-4, traj=True)
    assert tuple(w.shape) == (0, n) and tuple(tr.shape) == (steps, 0, n) and len(recorder.calls) == calls
    om = hebb_ops.hebb_noise(5, 2, 3, 4, 6, 7, n, t_dev=t_dev)
    assert recorder.calls[-1] == ("tnf_hebb_noise_f32", (om.data_ptr(), t_dev.data_ptr(), 5, 2, 3, 4, 6, 7, n, 0))
    assert tuple(om.shape) == (7, 4, n) and om.dtype == torch.float32
    hebb_ops.hebb_noise(5, 2, 3, 4, 6, 7, n)
    assert recorder.calls[-1][1][1] is None
    calls = len(recorder.calls)
    assert tuple(hebb_ops.hebb_noise(5, 2, 3, 0, 6, 7, n).shape) == (7, 0, n) and len(recorder.calls) == calls


def test_wrapper_refusals(recorder):
    z, x, w0 = torch.zeros(5, 4), torch.zeros(7, 20), torch.zeros(20)
    with pytest.raises(TypeError, match="float32 only"):
        hebb_ops.hebb_simulate(z.double(), x, w0, 3, 0.0)
    with pytest.raises(ValueError, match=r"z must be \(N, 4\)"):
        hebb_ops.hebb_simulate(torch.zeros(5, 3), x, w0, 3, 0.0)
    with pytest.raises(ValueError, match="x must be"):
        hebb_ops.hebb_simulate(z, torch.zeros(0, 20), w0, 3, 0.0)
    with pytest.raises(ValueError, match="1 <= n <= 64"):
        hebb_ops.hebb_simulate(z, torch.zeros(7, 65), torch.zeros(65), 3, 0.0)
    for bad in (torch.zeros(19), torch.zeros(2, 20), torch.zeros(1, 1, 20)):
        with pytest.raises(ValueError, match="w0 must be"):
            hebb_ops.hebb_simulate(z, x, bad, 3, 0.0)
    for bad in (-1, 2.0):
        with pytest.raises(ValueError, match="n_steps"):
            hebb_ops.hebb_simulate(z, x, w0, bad, 0.0)
    for bad in (-1e-4, float("nan")):
        with pytest.raises(ValueError, match="sigma_eps"):
            hebb_ops.hebb_simulate(z, x, w0, 3, bad)
    with pytest.raises(ValueError, match="eps must be"):
        hebb_ops.hebb_simulate(z, x, w0, 3, 0.0, eps=torch.zeros(3, 5, 19))
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="t_dev must be one int64"):
            hebb_ops.hebb_simulate(z, x, w0, 3, 0.0, t_dev=bad)
    with pytest.raises(ValueError, match="1 <= n <= 64"):
        hebb_ops.hebb_noise(0, 0, 0, 2, 0, 2, 0)
    assert not recorder.calls


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    np.random.seed(0)
    system = HebbLearn(5, 3)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        system.simulate(system.sample_prior(4))
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        system.sample_prior_device(4)
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        hebb_ops.hebb_noise(0, 0, 0, 2, 0, 2, 5)


# ---- systems.HebbLearn -----------------------------------------------------------------------------------------------------
def test_hebblearn_constructor_bounds_and_prior():
    np.random.seed(4)
    s = HebbLearn()
    assert (s.D, s.D_x, s.num_neurons, s.N_x, s.num_passes, s.n_steps, s.sigma_eps) == (4, 20, 20, 50, 2, 100, 1e-4)
    assert s.lb.tolist() == [1e-6, 1e-6, -4.0, 0.0] and s.ub.tolist() == [2e-1, 2e-1, 4.0, 20.0]
    assert type(s.support_layer) is tnf.ToInterval and s.support_layer.D == 4
    assert s.x.shape == (50, 20) and s.w0.shape == (20,) and np.isfinite(s.x).all() and 0 <= s.seed < 2 ** 31
    np.random.seed(4)
    again = HebbLearn()
    assert np.array_equal(again.x, s.x) and np.array_equal(again.w0, s.w0) and again.seed == s.seed  # np.random.seed governs
    assert HebbLearn(3, 2, 1, 0.0, seed=9).seed == 9 and HebbLearn(64, 1).x.shape == (1, 64)
    # x ~ N(0, Sigma), Sigma ~ IW(5 n, 5 n I): E[Sigma] = df / (df - n - 1) I, so the entries' variance is near 1.27
    big = HebbLearn(20, 4000)
    assert 1.0 < big.x.var() < 1.6 and abs(big.x.mean()) < 0.1
    for bad in (dict(num_neurons=0), dict(num_neurons=65), dict(num_neurons=20.0), dict(N_x=0), dict(num_passes=0),
                dict(sigma_eps=-1.0), dict(sigma_eps=float("nan"))):
        with pytest.raises(ValueError):
            HebbLearn(**bad)
    np.random.seed(5)
    z = s.sample_prior(4000)
    np.random.seed(5)
    assert z.shape == (4000, 4) and np.array_equal(z, s.prior.rvs(4000))
    lo, hi = np.array([1e-5, 1e-5, -3.0, 1.0]), np.array([1e-1, 1e-1, 3.0, 20.0])
    assert (z >= lo).all() and (z <= hi).all() and (z > s.lb).all() and (z < s.ub).all()  # inside the support layer's box
    assert abs(np.log10(z[:, 0]).mean() + 3.0) < 0.1 and abs(z[:, 3].mean() - 10.5) < 0.5
    lp = s.log_prior(z)
    assert np.array_equal(lp, s.prior.logpdf(z)) and np.isfinite(lp).all()
    # the density of the draw: 1 / (z ln10 4) per log-uniform coordinate, 1 / 6 and 1 / 19 for the uniform ones
    want = -np.log(z[:, 0] * np.log(10) * 4) - np.log(z[:, 1] * np.log(10) * 4) - np.log(6.0) - np.log(19.0)
    np.testing.assert_allclose(lp, want, rtol=0, atol=1e-13)  # sums of a few terms below 12 in float64: some 1e-15
    # ... which integrates to 1 over the box: int c / (a b) = c (ln 1e4)^2 * 6 * 19 in closed form
    c = np.exp(lp + np.log(z[:, 0]) + np.log(z[:, 1]))
    np.testing.assert_allclose(c * np.log(1e4) ** 2 * 6.0 * 19.0, 1.0, rtol=1e-12)
    outside = np.array([[1e-6, 1e-3, 0.0, 5.0], [1e-3, 0.2, 0.0, 5.0], [1e-3, 1e-3, 3.5, 5.0], [1e-3, 1e-3, 0.0, 0.5]])
    assert (s.log_prior(outside) == -np.inf).all()
    zt = torch.as_tensor(np.concatenate((z[:9], outside)))
    np.testing.assert_allclose(s.log_prior(zt).numpy(), s.log_prior(zt.numpy()), rtol=0, atol=1e-13)
    assert "not a density" in HebbLearn.__doc__ and "NOT the same stream" in HebbLearn.__doc__


def test_exports_and_torch_nf_aliases():
    for name in ("HebbLearn", "train_nde"):
        assert name in tnf.__all__ and hasattr(tnf, name)
    tnf.install_as_torch_nf()
    ns = {}
    exec("from torch_nf.systems import HebbLearn\nfrom torch_nf.lfi import train_nde", ns)
    assert ns["HebbLearn"] is HebbLearn and ns["train_nde"] is train_nde


def test_train_nde_argument_errors():
    np.random.seed(0)
    system = HebbLearn(5, 3)
    nf = tnf.NormFlow(4, True, "affine", support_layer=system.support_layer, device="cpu")
    cde = tnf.ConditionalDensityEstimator(nf, 5, [8])
    x0 = np.zeros((1, 5))
    for kw in (dict(N=0), dict(N=2.0), dict(R=0), dict(num_iters=0), dict(num_iters=-3)):
        with pytest.raises(ValueError, match="must be a positive int"):
            train_nde(cde, system, x0, **kw)
    for clip in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip must be None or positive"):
            train_nde(cde, system, x0, clip=clip)
    with pytest.raises(ValueError, match="must simulate on the device"):
        train_nde(cde, tnf.Mat(2), np.zeros((1, 2)))
    for bad in (np.zeros((1, 4)), np.zeros(5), np.zeros((2, 5))):
        with pytest.raises(ValueError, match=r"x0 must be \(1, D_x=5\)"):
            train_nde(cde, system, bad)


# ---- the restatement against the reference notebook's own function -----------------------------------------------------------
def _golden_noise(g):
    np.random.seed(int(g["noise_seed"]))
    return np.stack([np.random.normal(0.0, 1.0, (32, 20)) for _ in range(100)])


@pytest.mark.parametrize("order", H.ORDERS)
def test_restatement_reproduces_the_notebook(order):
    g = load_golden("hebb")
    assert g["z"].shape == (32, 4) and g["x"].shape == (50, 20) and g["steps"].tolist() == [0, 1, 49, 50, 99]
    for k in ("x", "w0", "z"):
        assert np.array_equal(g[k], g[k].astype(np.float32).astype(np.float64))  # what the kernel is handed is exact
    eps = _golden_noise(g)
    w, kept = H.simulate(g["z"], g["x"], g["w0"], eps, float(g["sigma_eps"]), order=order, keep=set(g["steps"].tolist()))
    benign = slice(0, 24)
    np.testing.assert_allclose(w[benign], g["w_final"][benign], rtol=1e-9, atol=0)
    for i, s in enumerate(g["steps"].tolist()):
        np.testing.assert_allclose(kept[s][benign], g["traj"][i][benign], rtol=1e-9, atol=0)
    for i, s in ((0, 0), (1, 1)):  # the whole-prior rows: chaotic later on, pinned where a step is still well conditioned
        np.testing.assert_allclose(kept[s][24:], g["traj"][i][24:], rtol=1e-9, atol=0)
    assert np.array_equal(kept[99], w) and np.array_equal(g["traj"][4], g["w_final"])


def test_restatement_conventions():
    rng = np.random.RandomState(2)
    x, w0 = H.inputs(rng, 7, 3)
    z = H.prior_rows(rng, 6)
    eps = rng.normal(0, 1, (7, 6, 7))
    full = H.trajectory(z, x, w0, eps, 1e-2)
    head = H.trajectory(z, x, w0, eps[:3], 1e-2)
    tail = H.trajectory(z, x, head[-1], eps[3:], 1e-2, j0=3)  # the x row cycles with the global step
    assert np.array_equal(full[:3], head) and np.array_equal(full[3:], tail)
    assert np.array_equal(H.simulate(z, x, w0, None, 0.0, n_steps=4)[0], H.simulate(z, x, w0, 0 * eps[:4], 0.0)[0])
    z[2, 0] = np.nan
    w, _ = H.simulate(z, x, w0, eps, 1e-2)
    assert np.isnan(w[2]).all() and np.isfinite(np.delete(w, 2, axis=0)).all()  # a NaN stays a NaN through the clips
    assert (np.abs(np.delete(w, 2, axis=0)) <= np.delete(z, 2, axis=0)[:, 3:4]).all()
    p = rng.normal(0, 1, (4, 21))
    for order in H.ORDERS:
        np.testing.assert_allclose(H.dot_rows(p, x[0, :1].repeat(21), order), (p * x[0, 0]).sum(1), rtol=1e-12)
    assert H.row_err(np.array([[1.0, 2.0]]), np.array([[1.0, 2.5]]), np.array([5.0])).tolist() == [0.1]
    assert H.row_err(np.array([[np.nan, 2.0]]), np.array([[np.nan, 2.0]]), np.array([5.0])).tolist() == [0.0]
    assert H.row_err(np.array([[np.nan, 2.0]]), np.array([[1.0, 2.0]]), np.array([5.0])).tolist() == [np.inf]
    box, clip = H.prior_rows(rng, 500, "box"), H.prior_rows(rng, 500, "clip")
    assert box[:, :2].max() <= 1e-2 and box[:, 3].min() >= 1.0 and 0.2 <= clip[:, 3].min() and clip[:, 3].max() <= 1.5
