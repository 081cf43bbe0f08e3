"""MoG without a GPU: the test oracle pinned to the reference's recorded outputs, the class's host-side behaviour, the
C-ABI argument checks of include/tnf_mog.h (no launches) and what the wrappers of mog_ops.py hand to the library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import mog_restatement as R

import torch_nf_amd as tnf
from torch_nf_amd import _lib, mog_ops, ops
from torch_nf_amd.density_estimator import MoG

CASES = [(2, 1), (2, 3), (5, 1), (5, 4), (8, 2), (16, 1)]
KEYS = ["d%dk%d%s_" % (D, K, b) for D, K in CASES for b in "ub"]


@pytest.fixture(scope="module")
def gold():
    return load_golden("mog")


def _case(gold, key):
    D, K = (16, 2) if key == "floor_" else tuple(int(v) for v in re.match(r"d(\d+)k(\d+)", key).groups())
    g = {n[len(key):]: v for n, v in gold.items() if n.startswith(key)}
    return D, K, g, g.get("lb"), g.get("ub")


# ---- the oracle is the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS + ["floor_"])
def test_restatement_reproduces_the_reference(gold, key):
    D, K, g, lb, ub = _case(gold, key)
    p64 = torch.tensor(g["params"].astype(np.float64), requires_grad=True)
    lp64 = R.log_prob(torch.tensor(g["z"].astype(np.float64)), p64, D, K, lb, ub)
    assert lp64.dtype == torch.float64
    np.testing.assert_allclose(lp64.detach().numpy(), g["lp64"], rtol=1e-12, atol=0)
    (gp,) = torch.autograd.grad((lp64 * torch.tensor(g["g_lp"])).sum(), p64)
    np.testing.assert_allclose(gp.numpy(), g["g_params"], rtol=1e-10, atol=1e-12 * np.abs(g["g_params"]).max())
    lp32 = R.log_prob(torch.tensor(g["z"]), torch.tensor(g["params"]), D, K, lb, ub)
    assert lp32.dtype == torch.float32
    ulp = np.spacing(np.float32(np.abs(g["lp32"]).max()))
    assert np.abs(lp32.numpy().astype(np.float64) - g["lp32"]).max() <= 2 * ulp
    got = R.mog_params(torch.tensor(g["params"]), D, K, lb, ub)
    for name, t in zip(("alpha", "mu", "Sigma_inv", "Sigma_det"), got):
        want = g[name]
        assert t.numpy().shape == want.shape
        assert np.abs(t.numpy().astype(np.float64) - want).max() <= 2 * np.spacing(np.float32(np.abs(want).max())), name
    if key == "floor_":
        assert np.abs(g["lp64"] - np.log(1e-12)).max() < 1e-9
    elif K > 1:
        assert g["lp64"].min() > -20.0


@pytest.mark.parametrize("key", KEYS)
def test_get_mog_params_and_log_prob_np(gold, key):
    D, K, g, lb, ub = _case(gold, key)
    mog = MoG(D, True, K, lb, ub, device="cpu")
    got = mog._get_MoG_params(torch.tensor(g["params"]))
    for name, t in zip(("alpha", "mu", "Sigma_inv", "Sigma_det"), got):
        want = g[name]
        assert tuple(t.shape) == want.shape
        np.testing.assert_allclose(t.numpy(), want, rtol=2e-6, atol=2e-6 * np.abs(want).max())
    a_np = mog._get_MoG_params(torch.tensor(g["params"]), numpy=True)[0]
    assert isinstance(a_np, np.ndarray) and np.allclose(a_np.sum(1), 1.0, atol=1e-7)
    lp = mog.log_prob_np(g["z"], torch.tensor(g["params"]))
    assert lp.dtype == np.float64 and lp.shape == g["lp64"].shape
    off_floor = g["lp64"] > -20.0  # where the density is far above EPS, the only place the two EPS placements agree
    assert off_floor.all() or (K == 1 and D == 16)  # a 16-dimensional Gaussian's own log-density is about -25
    # log(p + EPS) - log(p) <= EPS / p: the outer EPS, which the K == 1 branch of log_prob does not have, and twice
    # that for the EPS terms of log_prob's normalisers
    # with bounds the reference takes sqrt(m) in float32 even in its float64 run (m is a float32 tensor): a relative
    # 2^-24 in every U_ii, so 2^-23 q in the quadratic form (q < 2 |lp|) and 2^-24 D in the log-determinant
    base = 1e-9 if lb is None else 2.0 ** -23 * (D + 2 * np.abs(g["lp64"]))
    tol = base + 3e-12 * np.exp(-g["lp64"])
    assert np.all(np.abs(lp - g["lp64"])[off_floor] <= tol[off_floor])
    assert np.all(np.isfinite(lp))


# ---- the class ---------------------------------------------------------------------------------------------------------
def test_constructor_validation_and_counts():
    with pytest.raises(TypeError) as e:
        MoG(3, False, 2.0, device="cpu")
    assert "K" in str(e.value) and "int" in str(e.value)
    with pytest.raises(ValueError, match="MoG K 0 must be greater than 0."):
        MoG(3, False, 0, device="cpu")
    with pytest.raises(ValueError, match="DensityEstimator D 1 must be greater than 1."):
        MoG(1, False, 1, device="cpu")
    with pytest.raises(TypeError):
        MoG(3, 1, 1, device="cpu")
    for D, K in [(2, 1), (2, 3), (5, 4), (16, 1), (33, 2)]:
        want = K * (1 + D + D * (D + 1) // 2)
        mog = MoG(D, True, K, device="cpu")
        assert mog.D_params == want and _lib.lib.tnf_mog_num_params(D, K) == want and ops.mog_num_params(D, K) == want
        assert not hasattr(mog, "params")
    torch.manual_seed(3)
    mog = MoG(4, False, 3, device="cpu")
    assert tuple(mog.params.shape) == (1, mog.D_params) and mog.params.requires_grad and mog.params.dtype == torch.float32
    torch.manual_seed(3)
    want = torch.nn.init.xavier_normal_(torch.zeros(1, mog.D_params))
    assert torch.equal(mog.params.detach(), want)


def test_bounds_handling():
    lb, ub = np.array([-1.0, -2.0, 0.0]), np.array([1.0, 3.0, 0.5])
    assert MoG(3, True, 2, lb, None, device="cpu")._bounds() is None  # bounds apply only when both are given
    assert MoG(3, True, 2, None, ub, device="cpu")._bounds() is None
    b = MoG(3, True, 2, lb, ub, device="cpu")._bounds()
    assert b.dtype == torch.float32 and np.array_equal(b.numpy(), np.stack([lb, ub]).astype(np.float32))
    with pytest.raises(ValueError, match="shape"):
        MoG(3, True, 2, lb[:2], ub[:2], device="cpu")._bounds()
    with pytest.raises(ValueError, match="exceed"):
        MoG(3, True, 2, ub, lb, device="cpu")._bounds()
    mog = MoG(3, True, 2, lb, ub, device="cpu")
    _, mu, _, _ = mog._get_MoG_params(5.0 * torch.randn(4, mog.D_params))
    assert (mu >= torch.tensor(lb).float()).all() and (mu <= torch.tensor(ub).float()).all()


def test_install_as_torch_nf_exposes_mog():
    tnf.install_as_torch_nf()
    import torch_nf.density_estimator as de

    assert de.MoG is MoG and tnf.MoG is MoG and "MoG" in tnf.__all__


def test_cde_accepts_mog_only_exactly(monkeypatch):
    mog = MoG(3, True, 2, device="cpu")
    cde = tnf.ConditionalDensityEstimator(mog, 4, [8])
    assert cde.D_params == mog.D_params and cde.param_net[-1].out_features == mog.D_params

    class Sub(MoG):
        pass

    with pytest.raises(TypeError):
        tnf.ConditionalDensityEstimator(Sub(3, True, 2, device="cpu"), 4, [8])
    x = torch.zeros(20, 4)
    assert not cde._fused_conditioner_ok(torch.zeros(20, 1, 3), x) and not cde._fused_sampling_ok(x)
    calls = []
    monkeypatch.setattr(MoG, "__call__", lambda self, N=100, params=None: calls.append(("call", N, tuple(params.shape))))
    monkeypatch.setattr(MoG, "sample", lambda self, N=100, params=None, generator=None:
                        calls.append(("sample", N, tuple(params.shape))))
    cde(x, N=1, freeze_bn=True)  # a MoG takes no freeze_bn: passing it would be a TypeError here
    cde.sample(x, N=5)
    assert calls == [("call", 1, (20, mog.D_params)), ("sample", 5, (20, mog.D_params))]


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    mog = MoG(3, False, 2, device="cpu")
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        mog.log_prob(torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="needs a HIP device"):
        mog(N=3)


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_mog.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.MOG_SIGNATURES) and len(protos) == 7
    assert not set(_lib.MOG_SIGNATURES) & set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.MOG_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want, (name, p)
    assert '#include "tnf_mog.h"' in open(os.path.join(ROOT, "include", "tnf.h")).read()
    for n in ("MOG_COUNT_LOGPROB", "MOG_COUNT_LOGPROB_BWD", "MOG_COUNT_SAMPLE"):
        assert "TNF_%s = %d" % (n, getattr(_lib, n)) in open(os.path.join(ROOT, "include", "tnf_mog.h")).read()


def test_queries_host_side():
    lib = _lib.lib
    for K in (1, 2, 5, 26):
        for D in range(2, 17):
            assert lib.tnf_mog_supported(D, K) == 1
        assert lib.tnf_mog_supported(17, K) == 0 and lib.tnf_mog_supported(1, K) == 0
    assert lib.tnf_mog_supported(16, 27) == 0 and lib.tnf_mog_supported(5, 178) == 1 and lib.tnf_mog_supported(5, 0) == 0
    assert lib.tnf_mog_num_params(1, 1) == -1 and b"tnf_mog_num_params" in lib.tnf_last_error()
    assert lib.tnf_mog_num_params(5, 0) == -1 and lib.tnf_mog_num_params(4097, 1) == -1
    for which in range(3):
        assert lib.tnf_mog_launch_count(which) >= 0
    assert lib.tnf_mog_launch_count(3) == -1 and lib.tnf_mog_launch_count(-1) == -1
    P = 105
    assert lib.tnf_mog_bwd_workspace_bytes(1 << 16, 1 << 16, 1, 5, 5) == 0       # a lane owns a context's row
    assert lib.tnf_mog_bwd_workspace_bytes(1000, 1000, 64, 5, 5) == 0            # a workgroup owns a context's row
    assert lib.tnf_mog_bwd_workspace_bytes(1, 1, 1 << 20, 5, 5) == 256 * P * 4   # 256 partial rows
    assert lib.tnf_mog_bwd_workspace_bytes(1 << 10, 1, 1 << 10, 5, 5) == 256 * P * 4  # a shared row: one context of M N
    assert lib.tnf_mog_bwd_workspace_bytes(4, 4, 1000, 5, 5) == 4 * 8 * P * 4
    # the generic backward keeps its workgroups' arrays in the workspace, so it has no shape limit
    assert lib.tnf_mog_bwd_workspace_bytes(3, 3, 1, 36, 1) > 0 and lib.tnf_mog_bwd_workspace_bytes(1, 1, 129, 200, 3) > 0
    assert 0 < lib.tnf_mog_bwd_workspace_bytes(1 << 16, 1 << 16, 1, 33, 1) < 1 << 29
    assert lib.tnf_mog_bwd_workspace_bytes(3, 3, 0, 5, 5) == 0
    assert lib.tnf_mog_bwd_workspace_bytes(2, 3, 4, 5, 5) == -1 and lib.tnf_mog_bwd_workspace_bytes(1, 1, 4, 1, 5) == -1


def test_argument_refusals_without_launching():
    lib = _lib.lib
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    INV, WS = -1, -4
    P = 105

    def lp(**kw):
        a = dict(z=p[0], params=p[1], bounds=None, lp=p[2], Mz=3, Mp=3, N=4, D=5, K=5, ld=P)
        a.update(kw)
        return lib.tnf_mog_log_prob_f32(a["z"], a["params"], a["bounds"], a["lp"], a["Mz"], a["Mp"], a["N"], a["D"], a["K"],
                                        a["ld"], None)

    def bwd(**kw):
        a = dict(z=p[0], params=p[1], bounds=None, g=p[2], gz=None, gp=p[3], Mz=1, Mp=1, N=1 << 20, D=5, K=5, ld=P, ws=p[4],
                 wsb=1 << 30)
        a.update(kw)
        return lib.tnf_mog_log_prob_backward_f32(a["z"], a["params"], a["bounds"], a["g"], a["gz"], a["gp"], a["Mz"],
                                                 a["Mp"], a["N"], a["D"], a["K"], a["ld"], a["ws"], a["wsb"], None)

    def smp(**kw):
        a = dict(params=p[0], u=p[1], e1=p[2], e2=p[3], z=p[4], lq=p[5], M=3, N=4, D=5, K=5, ld=P)
        a.update(kw)
        return lib.tnf_mog_sample_f32(a["params"], None, a["u"], a["e1"], a["e2"], a["z"], a["lq"], a["M"], a["N"], a["D"],
                                      a["K"], a["ld"], None)

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, msg)

    for name in ("z", "params", "lp"):
        refused(lp(**{name: None}), INV, b"tnf_mog_log_prob_f32: NULL pointer")
    refused(lp(Mz=2, Mp=3), INV, b"do not broadcast")
    refused(lp(Mz=3, Mp=2), INV, b"do not broadcast")
    refused(lp(Mz=0), INV, b"bad batch sizes")
    refused(lp(N=-1), INV, b"bad batch sizes")
    refused(lp(ld=P - 1), INV, b"params row has 104 elements, MoG(D=5, K=5) needs 105")
    refused(lp(D=1), INV, b"tnf_mog_log_prob_f32: D=1 K=5")
    refused(lp(K=0), INV, b"tnf_mog_log_prob_f32: D=5 K=0")
    for name in ("z", "params", "g", "gp"):
        refused(bwd(**{name: None}), INV, b"tnf_mog_log_prob_backward_f32: NULL pointer")
    refused(bwd(Mz=2, Mp=3), INV, b"do not broadcast")
    refused(bwd(ld=10), INV, b"params row has 10 elements")
    refused(bwd(wsb=256 * P * 4 - 1), WS, b"tnf_mog_log_prob_backward_f32: workspace")
    refused(bwd(ws=None), WS, b"workspace")
    refused(bwd(ws=ctypes.c_void_p(4096 + 8)), INV, b"16-byte aligned")
    for name in ("params", "u", "e1", "e2", "z", "lq"):
        refused(smp(**{name: None}), INV, b"tnf_mog_sample_f32: NULL pointer")
    refused(smp(ld=P - 1), INV, b"params row has 104 elements")
    refused(smp(M=0), INV, b"bad batch sizes")
    refused(smp(D=4097), INV, b"tnf_mog_sample_f32: D=4097 K=5")


# ---- what the wrappers hand over ---------------------------------------------------------------------------------------
class _Recorder(object):
    """Stands in for mog_ops.lib: queries go to the library, compute entries are noted and answer 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        real = getattr(_lib.lib, name)
        if name in ("tnf_mog_num_params", "tnf_mog_bwd_workspace_bytes", "tnf_mog_supported"):
            return real

        def call(*args):
            assert len(args) == len(_lib.MOG_SIGNATURES[name][1]), name
            self.calls.append((name, args))
            return 0

        return call


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "require_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    monkeypatch.setattr(mog_ops, "lib", rec)
    ops._ws_cache.clear()
    yield rec
    ops._ws_cache.clear()


def test_wrapper_marshalling(recorder):
    D, K, P = 5, 5, 105
    wide = torch.zeros(3, P + 6, requires_grad=True)
    params = wide[:, 2:2 + P]  # a slice of a wider tensor: passed as it is, with its row stride
    z = torch.zeros(3, 4, D, requires_grad=True)
    bounds = torch.tensor([[-1.0] * D, [1.0] * D])
    lp = ops.mog_log_prob(z, params, D, K, bounds)
    assert tuple(lp.shape) == (3, 4) and lp.dtype == torch.float32 and lp.requires_grad
    name, a = recorder.calls[-1]
    assert name == "tnf_mog_log_prob_f32"
    assert a[0] == z.data_ptr() and a[1] == params.data_ptr() and a[2] is not None and a[4:] == (3, 3, 4, D, K, P + 6, 0)
    gz, gp = torch.autograd.grad(lp.sum(), [z, wide])
    name, a = recorder.calls[-1]
    assert name == "tnf_mog_log_prob_backward_f32" and a[6:12] == (3, 3, 4, D, K, P + 6) and a[12] is None and a[13] == 0
    assert tuple(gz.shape) == (3, 4, D) and tuple(gp.shape) == (3, P + 6)
    # one shared row and many samples: partial rows in a workspace of ops._workspace; g_z not wanted -> NULL
    p1 = torch.zeros(1, P, requires_grad=True)
    lp = ops.mog_log_prob(torch.zeros(2, 300, D), p1, D, K)
    torch.autograd.grad(lp.sum(), [p1])
    name, a = recorder.calls[-1]
    need = _lib.lib.tnf_mog_bwd_workspace_bytes(2, 1, 300, D, K)
    assert need == 5 * P * 4 and a[2] is None and a[4] is None and a[6:9] == (2, 1, 300)
    buf = list(ops._ws_cache.values())[0]
    assert a[12] == buf.data_ptr() and a[13] == buf.numel() >= need
    # a broadcast z: its gradient is summed over the contexts
    zb = torch.zeros(1, 4, D, requires_grad=True)
    (gz,) = torch.autograd.grad(ops.mog_log_prob(zb, params, D, K).sum(), [zb])
    assert tuple(gz.shape) == (1, 4, D)
    n = len(recorder.calls)
    assert tuple(ops.mog_log_prob_raw(torch.zeros(3, 0, D), params, D, K).shape) == (3, 0) and len(recorder.calls) == n
    zs, lq = ops.mog_sample_raw(params.detach(), torch.zeros(3, 4), torch.zeros(3, 4, D), torch.zeros(3, 4, D), D, K)
    name, a = recorder.calls[-1]
    assert name == "tnf_mog_sample_f32" and a[7:] == (3, 4, D, K, P + 6, 0) and a[1] is None
    assert tuple(zs.shape) == (3, 4, D) and tuple(lq.shape) == (3, 4) and zs.dtype == lq.dtype == torch.float32


def test_wrapper_refusals(recorder):
    D, K, P = 5, 5, 105
    with pytest.raises(TypeError, match="float32 only"):
        ops.mog_log_prob(torch.zeros(1, 2, D, dtype=torch.float64), torch.zeros(1, P, dtype=torch.float64), D, K)
    with pytest.raises(TypeError, match="float32 only"):
        ops.mog_log_prob(torch.zeros(1, 2, D), torch.zeros(1, P, dtype=torch.float16), D, K)
    with pytest.raises(ValueError, match="D_params=105"):
        ops.mog_log_prob(torch.zeros(1, 2, D), torch.zeros(1, P + 1), D, K)
    with pytest.raises(ValueError, match="must be"):
        ops.mog_log_prob(torch.zeros(2, D), torch.zeros(1, P), D, K)
    with pytest.raises(RuntimeError, match="do not broadcast"):
        ops.mog_log_prob(torch.zeros(2, 2, D), torch.zeros(3, P), D, K)
    with pytest.raises(ValueError, match="bounds must be"):
        ops.mog_log_prob(torch.zeros(1, 2, D), torch.zeros(1, P), D, K, torch.zeros(2, D + 1))
    with pytest.raises(ValueError, match="draws must be"):
        ops.mog_sample_raw(torch.zeros(3, P), torch.zeros(3, 5), torch.zeros(3, 4, D), torch.zeros(3, 4, D), D, K)
    assert not recorder.calls
