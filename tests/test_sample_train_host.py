"""Training through frozen-statistics sampling in one backward kernel (include/tnf_sampletrain.h), without a GPU:
header, exports and binding table in step; the support predicate and the workspace query over a grid; every refusal that
precedes a launch; the routing of NormFlow with the switch `sample_training` on and off; and the algebra of the kernel's
walk (tests/sampletrain_restatement.py) against float64 autograd through the oracle."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import sampletrain_restatement as R
import test_route_table as RT
from domain_helpers import float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, sampletrain_ops

lib = _lib.lib
INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
NAMES = ("tnf_flow_sample_train_supported", "tnf_flow_sample_train_workspace_bytes", "tnf_sampletrain_launch_count",
         "tnf_flow_sample_bwd_f32")
TOL64 = dict(rtol=1e-9, atol=1e-9)  # the project's float64 tolerance (tests/test_gpu_grad.py)


# ---- the algebra of the walk, before any kernel --------------------------------------------------------------------------
def problem(oracle, D, S, L, U, M, Mp, N, seed=0):
    """float64 (omega, params (Mp, P), [(mean, alpha)] x 2S with non-trivial values, G, gamma)."""
    g = torch.Generator().manual_seed(seed)
    P = oracle.flow_num_params(D, S, L, U)
    params = torch.randn(Mp, P, generator=g, dtype=torch.float64) * 0.2
    stats = [(torch.randn(D, generator=g, dtype=torch.float64) * 0.3, torch.rand(D, generator=g, dtype=torch.float64) + 0.5)
             for _ in range(2 * S)]
    omega = torch.randn(M, N, D, generator=g, dtype=torch.float64)
    return omega, params, stats, torch.randn(M, N, D, generator=g, dtype=torch.float64), \
        torch.randn(M, N, generator=g, dtype=torch.float64)


def oracle_grad(oracle, omega, params, stats, G, gamma, D, S, L, U):
    """(z, d loss / d params) of loss = sum z G + sum sum_log_det gamma by float64 autograd over oracle.flow_forward."""
    with float64():
        p = params.clone().requires_grad_()
        z, log_q, _ = oracle.flow_forward(omega.numpy(), p, D, S, L, U, bn_stats=stats)
        sld = torch.tensor(oracle.base_log_density_f64(omega.numpy())) - log_q
        ((z * G).sum() + (sld * gamma).sum()).backward()
    return z.detach(), p.grad


@pytest.mark.parametrize("Mp", [1, 2])
@pytest.mark.parametrize("D,S,L,U", [(2, 1, 1, 15), (5, 2, 2, 15), (8, 2, 3, 16), (32, 2, 2, 15)])
def test_restatement_against_float64_autograd(oracle, D, S, L, U, Mp):
    M, N = 2, 7
    omega, params, stats, G, gamma = problem(oracle, D, S, L, U, M, Mp, N, seed=D + Mp)
    z, want = oracle_grad(oracle, omega, params, stats, G, gamma, D, S, L, U)
    mean, alpha = torch.stack([m for m, _ in stats]), torch.stack([a for _, a in stats])
    got_omega, got = R.sample_bwd(z, params, mean, alpha, G, gamma, D, S, L, U)
    assert got.shape == params.shape and got_omega.shape == omega.shape
    torch.testing.assert_close(got_omega, omega, **TOL64)
    torch.testing.assert_close(got, want, **TOL64)
    # each cotangent alone: the other absent is the other zero
    for G1, g1 in ((G, torch.zeros_like(gamma)), (torch.zeros_like(G), gamma)):
        _, want1 = oracle_grad(oracle, omega, params, stats, G1, g1, D, S, L, U)
        torch.testing.assert_close(R.sample_bwd(z, params, mean, alpha, G1, g1, D, S, L, U)[1], want1, **TOL64)


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_sampletrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.SAMPLETRAIN_SIGNATURES) == sorted(NAMES) and len(protos) == 4
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES) | set(_lib.PADTRAIN_SIGNATURES) | set(_lib.PADBATCH_SIGNATURES)
              | set(_lib.CTXFLOW_SIGNATURES) | set(_lib.CTXTRAIN_SIGNATURES))
    assert not set(_lib.SAMPLETRAIN_SIGNATURES) & others  # disjoint from the other nine
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.SAMPLETRAIN_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.SAMPLETRAIN_SIGNATURES["tnf_sampletrain_launch_count"][0] is ctypes.c_int64
    assert _lib.SAMPLETRAIN_SIGNATURES["tnf_flow_sample_train_workspace_bytes"][0] is ctypes.c_int64
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_sampletrain.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    assert _lib.DIAG_FAMILIES == 19  # a counter of its own: the flow families are a closed set
    assert lib.tnf_sampletrain_launch_count() >= 0


def test_supported_is_the_union_of_the_two_training_predicates():
    ones = 0
    for D in range(1, 67):
        for S in (1, 4, 9):
            for L in range(1, 5):
                for U in (15, 16, 17):
                    want = int(lib.tnf_flow_train_rev_supported(D, S, L, U) == 1
                               or lib.tnf_flow_padded_train_supported(D, S, L, U) == 1)
                    assert lib.tnf_flow_sample_train_supported(D, S, L, U) == want, (D, S, L, U)
                    if want:
                        assert (D in (32, 64)) == (lib.tnf_flow_train_rev_supported(D, S, L, U) == 1)
                        assert 2 <= D <= 64 and L <= 3 and U <= 16
                    ones += want
    assert ones > 200  # not vacuous
    assert lib.tnf_flow_sample_train_supported(64, 4, 2, 15) == 1 and lib.tnf_flow_sample_train_supported(5, 2, 2, 15) == 1
    assert lib.tnf_flow_sample_train_supported(65, 4, 2, 15) == 0 and lib.tnf_flow_sample_train_supported(1, 1, 1, 15) == 0
    assert sampletrain_ops.flow_sample_train_supported(1, 1, 64, 64, 4, 2, 15)
    assert sampletrain_ops.flow_sample_train_supported(3, 3, 32, 5, 2, 2, 15)
    assert not sampletrain_ops.flow_sample_train_supported(3, 3, 31, 5, 2, 2, 15)  # per-context rows need 32 samples
    assert sampletrain_ops.flow_sample_train_supported(3, 1, 1, 5, 2, 2, 15)
    assert not sampletrain_ops.flow_sample_train_supported(3, 2, 64, 5, 2, 2, 15)  # M_p not in {1, M}


def test_workspace_query():
    q = lib.tnf_flow_sample_train_workspace_bytes
    for D, S, L, U in ((64, 4, 2, 15), (32, 2, 3, 16), (5, 2, 2, 15), (63, 1, 1, 15), (2, 8, 2, 15)):
        sizes = [q(1, 1, N, D, S, L, U) for N in (1, 300, 1 << 12, 1 << 16)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], (D, sizes)
        assert q(3, 3, 64, D, S, L, U) > 0 and q(3, 1, 64, D, S, L, U) > 0
    for S, L, U in ((2, 2, 15), (2, 3, 16), (1, 1, 15)):  # the embedded problem of D = 5 is the D = 32 one
        for N in (1, 37, 4096):
            assert q(1, 1, N, 5, S, L, U) >= q(1, 1, N, 32, S, L, U) > 0
            assert q(1, 1, N, 33, S, L, U) >= q(1, 1, N, 64, S, L, U) > 0
    for D, S, L, U in ((65, 4, 2, 15), (1, 1, 1, 15), (64, 4, 4, 15), (64, 4, 2, 17), (5, 2, 2, 20), (64, 40, 2, 15)):
        assert q(1, 1, 64, D, S, L, U) == UNSUP, (D, S, L, U)
    for M, Mp, N in ((0, 1, 64), (3, 2, 64), (1, 1, -1)):
        assert q(M, Mp, N, 64, 4, 2, 15) == INV
    assert q(1, 1, 0, 64, 4, 2, 15) > 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]  # never dereferenced: every call fails validation first
    count = sampletrain_ops.sample_train_launch_count()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]
    pad = [lib.tnf_padtrain_launch_count(i) for i in range(5)]
    tag = b"tnf_flow_sample_bwd_f32"

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    for D, S in ((64, 4), (5, 2)):
        P = lib.tnf_flow_num_params(D, S, 2, 15)
        big = 1 << 40

        def bwd(**kw):
            a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], g_z=p[4], g_sld=p[5], g_params=p[6], omega=p[7], M=3, Mp=3,
                     N=64, D=D, S=S, L=2, U=15, pstride=P, gpstride=P, ws=p[8], ws_bytes=big)
            a.update(kw)
            return lib.tnf_flow_sample_bwd_f32(a["z"], a["params"], a["mean"], a["alpha"], a["g_z"], a["g_sld"], a["g_params"],
                                               a["omega"], a["M"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"],
                                               a["pstride"], a["gpstride"], a["ws"], a["ws_bytes"], None, None)

        for name in ("z", "params", "mean", "alpha", "g_params"):
            refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
        refused(bwd(g_z=None, g_sld=None), INV, tag + b": g_z and g_sld are both NULL")
        for kw in (dict(M=0), dict(M=-3), dict(Mp=2), dict(Mp=0), dict(N=-1), dict(M=1, Mp=3)):
            refused(bwd(**kw), INV, tag + b": M=")
        for kw in (dict(D=1), dict(D=65), dict(D=0), dict(L=4), dict(L=0), dict(U=17), dict(U=0), dict(S=0), dict(S=40)):
            refused(bwd(**kw), UNSUP, tag + b": no sampling backward for D=")
        refused(bwd(pstride=P - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P - 1, P))
        refused(bwd(gpstride=P - 1), INV, tag + b": g_params row too short")
        refused(bwd(g_params=p[1]), INV, tag + b": g_params must not alias params")
        refused(bwd(omega=p[0]), INV, tag + b": omega_out must not alias z")
        need = lib.tnf_flow_sample_train_workspace_bytes(3, 3, 64, D, S, 2, 15)
        assert need > 0
        for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
            assert bwd(**kw) == WS and tag in lib.tnf_last_error()
        assert bwd(N=0) == 0 and bwd(N=0, omega=None, g_z=None) == 0  # nothing to do: OK, no launch
        refused(bwd(N=0, gpstride=P - 1), INV, tag + b": g_params row too short")  # ... after the other checks
    assert sampletrain_ops.sample_train_launch_count() == count  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag
    assert [lib.tnf_padtrain_launch_count(i) for i in range(5)] == pad


# ---- routing: the recorder technique of tests/test_route_table.py, with the new module's entry recorded -----------------
TRAIN = "flow_sample_train"


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.sample_training` = switch (None: the class default) and the new entry
    recorded."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is not None:
            mp.setattr(tnf.NormFlow, "sample_training", switch)
        trace = []

        def recorder(*args, **kwargs):
            trace.append(TRAIN)
            raise RT._Reached()

        mp.setattr(sampletrain_ops, TRAIN, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


TAKES = [dict(D=D, M=1, N=64) for D in (64, 32, 5, 48, 33)] + [dict(D=D, rows="M", M=3, N=32) for D in (64, 32, 5, 48, 33)]
STAYS = [dict(no_grad=True), dict(freeze_bn=False), dict(arch="AR", S=1, D=5), dict(U=20), dict(fusion="LAYER"),
         dict(stats_graph=True), dict(rows="M", M=3, N=31), dict(p_grad=False), dict(arch="affine", S=1),
         dict(rows="M", M=3, N=31, D=5), dict(D=5, fusion="LAYER"), dict(D=5, U=20), dict(D=5, no_grad=True)]
_ids = lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "default"  # noqa: E731


@pytest.mark.parametrize("kw", TAKES, ids=_ids)
def test_forward_with_a_parameter_gradient_routes_to_train_sample(kw):
    r = RT.row(**dict(dict(op="forward", p_grad=True), **kw))
    old = RT._table()[RT.row_id(r)]
    assert run_row(r, False) == old and run_row(r, None) == old  # off, and by default: today's route
    assert old[-1] == "coupling"  # the per-bijector composition is what the family takes over
    assert run_row(r, True) == old[:-1] + [TRAIN]
    for draw in ("torch32", "torch64"):
        assert run_row(dict(r, draw=draw), True)[-1] == TRAIN


@pytest.mark.parametrize("kw", STAYS, ids=_ids)
def test_exclusions_run_what_they_run_today(kw):
    r = RT.row(**dict(dict(op="forward", p_grad=True), **kw))
    on, today = run_row(r, True), run_row(r, False)
    assert on == today and TRAIN not in on, (on, today)
    if RT.row_id(r) in RT._table():
        assert today == RT._table()[RT.row_id(r)]


def test_log_prob_inverse_and_the_switch_off_over_the_whole_grid():
    """Switch off: every row equals its entry of tests/route_table.json.  Switch on: a row changes only if it is a
    frozen-statistics forward, and then only in its last entry; log_prob and inverse never change."""
    table, changed = RT._table(), 0
    for i, r in enumerate(RT.GRID):
        old = table[RT.row_id(r)]
        candidate = r["op"] == "forward" and r["freeze_bn"] and r["p_grad"] and not r["no_grad"]
        if not candidate and i % 7:  # every candidate row, every seventh of the others
            continue
        assert run_row(r, False) == old, RT.row_id(r)
        on = run_row(r, True)
        if on != old:
            assert candidate and r["arch"] == "coupling" and r["U"] <= 16 and r["fusion"] != "LAYER" and not r["stats_graph"]
            assert not (r["rows"] == "M" and r["M"] > 1 and r["N"] < 32)  # (`zdtype` is the z of log_prob / inverse)
            # (a float32 tensor draw: log_q comes from the forward kernel, as on `padded`; no separate base density)
            kept = [t for t in old[:-1] if not (r["draw"] == "torch32" and t == "base_log_density_f64")]
            assert old[-1] == "coupling" and on == kept + [TRAIN], RT.row_id(r)
            changed += 1
    assert changed >= 10, changed  # not vacuous


def test_family_and_its_exclusions():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    om, p = torch.zeros(3, 32, 5), torch.zeros(3, nf.D_params, requires_grad=True)
    assert tnf.NormFlow.sample_training is False and nf.sample_training is False
    assert nf._route("forward", om, p).family == "bijectors"  # the switch defaults to off
    nf.sample_training = True
    assert nf._route("forward", om, p) == ("train_sample", False, False)
    assert nf._route("forward", om, p, f32_draw=True) == ("train_sample", False, True)  # log_q from the kernel, as `padded`
    assert nf._route("forward", om[:1], p[:1]).family == "train_sample"  # one shared row: any N
    assert nf._route("forward", om[:1, :1], p[:1]).family == "train_sample"
    assert nf._route("forward", om[:, :31], p).family == "bijectors"  # per-context rows need 32 samples
    assert nf._route("forward", om, p, freeze_bn=False).family != "train_sample"  # fresh statistics: their own families
    assert nf._route("forward", om, p.detach()).family == "padded"  # nothing to train: the inference kernel
    with torch.no_grad():
        assert nf._route("forward", om, p).family == "padded"
    assert nf._route("log_prob", om, p).family != "train_sample" and nf._route("inverse", om, p).family != "train_sample"
    assert nf._route("forward", om.double(), p).family == "bijectors"
    assert nf._route("forward", om[0], p).family == "bijectors"  # 2-d
    nf.fusion = _lib.FUSE_LAYER
    assert nf._route("forward", om, p).family == "bijectors"
    nf.fusion = _lib.FUSE_FLOW
    assert nf._route("forward", om, p).family == "train_sample"
    nf.fusion = _lib.FUSE_AUTO
    for b in nf._bn_layers():  # statistics in the graph: only the composition differentiates through them
        b._last_mean = torch.zeros(5, requires_grad=True)
        break
    assert nf._route("forward", om, p).family == "bijectors"
    ar = tnf.NormFlow(5, True, "AR", 1, 2, 15, device="cpu")
    ar.sample_training = True
    assert ar._route("forward", om, torch.zeros(3, ar.D_params, requires_grad=True)).family != "train_sample"
    wide = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
    wide.sample_training = True
    assert wide._route("forward", om, torch.zeros(3, wide.D_params, requires_grad=True)).family == "bijectors"  # U > 16
    sup = tnf.NormFlow(4, True, "coupling", 2, 2, 15, tnf.ToInterval(4, [-1.0] * 4, [2.0] * 4), device="cpu")
    sup.sample_training = True
    ps = torch.zeros(1, sup.D_params, requires_grad=True)
    assert sup._route("forward", torch.zeros(1, 8, 4), ps) == ("train_sample", False, False)  # the support layer: its own op
    d64 = tnf.NormFlow(64, True, "coupling", 4, 2, 15, device="cpu")
    d64.sample_training = True
    p64 = torch.zeros(1, d64.D_params, requires_grad=True)
    assert d64._route("forward", torch.zeros(1, 300, 64), p64).family == "train_sample"
    assert d64._route("forward", torch.zeros(1, 300, 64), p64.detach()).family == "fused"


def test_stats_walk_runs_at_most_once_per_call(monkeypatch):
    calls = []
    real = tnf.NormFlow._stats_in_graph
    monkeypatch.setattr(tnf.NormFlow, "_stats_in_graph", lambda self: (calls.append(1), real(self))[1])
    for kw in TAKES + STAYS:
        del calls[:]
        run_row(RT.row(**dict(dict(op="forward", p_grad=True), **kw)), True)
        assert len(calls) <= 1, (kw, len(calls))
