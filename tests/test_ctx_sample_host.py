"""Training per-context coupling flows with fewer than 32 draws per context through their frozen-statistics samples in one
backward launch (include/tnf_ctxsample.h), without a GPU: header, exports and binding table in step; the support
predicate over a grid against its definition; every refusal that precedes a launch; the routing of NormFlow with the
switch `context_sample_training` on, off and absent; and the algebra of the kernel's walk
(tests/ctxsample_restatement.py) against float64 autograd through the oracle's composition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, grad_err
import ctxsample_restatement as R
import test_gpu_ctx_flow as CF
import test_route_table as RT
from domain_helpers import BAR_P, BAR_Z, float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, ctxflow_ops, ctxsample_ops, ctxtrain_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
NAMES = ("tnf_ctx_sample_supported", "tnf_ctx_sample_launch_count", "tnf_ctx_sample_bwd_f32")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_ctxsample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.CTXSAMPLE_SIGNATURES) == sorted(NAMES) and len(protos) == 3
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES) | set(_lib.PADTRAIN_SIGNATURES) | set(_lib.PADBATCH_SIGNATURES)
              | set(_lib.CTXFLOW_SIGNATURES) | set(_lib.CTXTRAIN_SIGNATURES) | set(_lib.SAMPLETRAIN_SIGNATURES)
              | set(_lib.ARSAMPLE_SIGNATURES) | set(_lib.ARBATCH_SIGNATURES))
    assert not set(_lib.CTXSAMPLE_SIGNATURES) & others  # disjoint from the other twelve
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.CTXSAMPLE_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.CTXSAMPLE_SIGNATURES["tnf_ctx_sample_launch_count"][0] is ctypes.c_int64
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_ctxsample.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    assert _lib.DIAG_FAMILIES == 19  # a counter of its own: the flow families are a closed set
    assert lib.tnf_ctx_sample_launch_count() >= 0


def test_predicate_is_its_definition_over_the_grid():
    ones = 0
    for D in (-1, 0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 66):
        for S in (0, 1, 4, 40):
            for L in range(0, 5):
                for U in (0, 1, 15, 16, 17):
                    for N in (-1, 0, 1, 16, 31, 32, 33):
                        want = 2 <= D <= 64 and S >= 1 and 1 <= L <= 3 and 1 <= U <= 16 and 1 <= N <= 31
                        assert lib.tnf_ctx_sample_supported(D, S, L, U, N) == int(want), (D, S, L, U, N)
                        assert lib.tnf_ctx_train_supported(D, S, L, U, N) == int(want)  # the stated domain
                        assert lib.tnf_ctx_flow_supported(D, S, L, U, N) == int(want)  # ... and the forward half's
                        assert ctxsample_ops.ctx_sample_supported(D, S, L, U, N) == want
                        ones += want
    assert ones == 7 * 3 * 3 * 3 * 3
    assert lib.tnf_ctx_sample_supported(64, 1000, 3, 16, 31) == 1  # no bound on S: one layer's block at a time
    assert lib.tnf_ctx_sample_supported(5, 2, 2, 15, 1 << 40) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    count, t_count, counts = ctxsample_ops.launch_count(), ctxtrain_ops.launch_count(), ctxflow_ops.launch_counts()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]
    tag = b"tnf_ctx_sample_bwd_f32"

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 15)

    def bwd(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], g_z=p[4], g_sld=p[5], g_params=p[6], g_omega=p[7], M=3, N=8,
                 D=5, S=2, L=2, U=15, pstride=P5, gpstride=P5)
        a.update(kw)
        return lib.tnf_ctx_sample_bwd_f32(a["z"], a["params"], a["mean"], a["alpha"], a["g_z"], a["g_sld"], a["g_params"],
                                          a["g_omega"], a["M"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                          a["gpstride"], None)

    for name in ("z", "params", "mean", "alpha", "g_params"):
        refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
    refused(bwd(g_z=None, g_sld=None), INV, tag + b": no upstream gradient")
    refused(bwd(g_z=None, g_sld=None, g_omega=None), INV, tag + b": no upstream gradient")
    for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
        refused(bwd(**kw), INV, tag + b": M=")
    refused(bwd(M=1 << 31), INV, tag + b": M=2147483648 exceeds the grid")
    for kw in (dict(D=1), dict(D=65), dict(D=0), dict(L=4), dict(L=0), dict(U=17), dict(U=0), dict(S=0), dict(N=32),
               dict(N=1000)):
        refused(bwd(**kw), UNSUP, tag + b": no per-context kernel for D=")
    refused(bwd(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(gpstride=P5 - 1), INV, tag + b": gradient row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(pstride=0), INV, tag + b": params row has 0 elements")
    refused(bwd(g_omega=p[0]), INV, tag + b": g_omega must not alias z or g_z")
    refused(bwd(g_omega=p[4]), INV, tag + b": g_omega must not alias z or g_z")
    refused(bwd(g_params=p[1]), INV, tag + b": g_params must not alias params")
    assert bwd(N=0) == 0 and bwd(N=0, g_omega=None) == 0 and bwd(N=0, g_z=None) == 0  # nothing to do: OK, no launch
    refused(bwd(N=0, gpstride=P5 - 1), INV, tag + b": gradient row has")  # ... after the other checks
    # every supported shape's slice fits 64 KB (the largest, D = 64, L = 3, U = 16, N = 31, is 49,280 bytes), so the
    # slice refusal is unreachable through the predicate's domain: nothing to provoke here
    assert ctxsample_ops.launch_count() == count and ctxtrain_ops.launch_count() == t_count
    assert ctxflow_ops.launch_counts() == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing: the method of tests/test_ctx_train_host.py, with the new entry recorded ------------------------------------
TRAIN = "ctx_flow_sample_train"
SWITCH = "context_sample_training"


def run_row(r, switch, others=None):
    """test_route_table.run_row with `NormFlow.context_sample_training` = switch (None: the attribute absent, as on the
    parent commit), `context_rows` and `context_training` = others, and the new entry recorded beside those of
    ctxflow_ops and ctxtrain_ops."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is None:
            mp.delattr(tnf.NormFlow, SWITCH, raising=False)
        else:
            mp.setattr(tnf.NormFlow, SWITCH, switch, raising=False)
        if others is not None:
            mp.setattr(tnf.NormFlow, "context_rows", others, raising=False)
            mp.setattr(tnf.NormFlow, "context_training", others, raising=False)
        trace = []
        for mod, name in ((ctxsample_ops, TRAIN), (ctxtrain_ops, "ctx_flow_log_prob_train"),
                          (ctxflow_ops, "ctx_flow_log_prob_raw"), (ctxflow_ops, "ctx_flow_forward_raw")):
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(mod, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_context_sample_training(r):
    """The conditions of the new row of the routing docstring, from the grid row alone.  (The grid's parameters are
    float32, and a forward's draw becomes float32 with one block per parameter row, whatever its dtype.)"""
    return (r["op"] == "forward" and r["freeze_bn"] and r["arch"] == "coupling" and not r["no_grad"] and r["p_grad"]
            and not r["stats_graph"] and r["rows"] == "M" and r["M"] > 1 and r["fusion"] != "LAYER"
            and lib.tnf_ctx_sample_supported(r["D"], r["S"], RT.L, r["U"], r["N"]) == 1)


def test_every_row_of_the_grid_on_off_and_absent():
    """Switch off or absent: every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of the new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), 0
    for r in RT.GRID:
        old = table[RT.row_id(r)]
        want = takes_context_sample_training(r)
        assert run_row(r, False) == old, RT.row_id(r)
        if want or not RT.GRID.index(r) % 5:  # the attribute absent: every candidate row, every fifth of the others
            assert run_row(r, None) == old, RT.row_id(r)
        on = run_row(r, True)
        if want:
            assert old[-1] == "coupling", RT.row_id(r)  # nothing another family takes changes hands
            assert on == old[:-1] + [TRAIN], RT.row_id(r)
            assert run_row(r, True, others=True) == on  # independent of context_rows and context_training
            assert run_row(r, False, others=True) == old  # ... which leave sampling under autograd alone
            changed += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed >= 10, changed  # not vacuous


@pytest.mark.parametrize("kw", [dict(rows="one", M=1, N=31), dict(rows="one", M=3, N=31), dict(N=32), dict(N=64),
                                dict(arch="AR", S=1), dict(fusion="LAYER"), dict(stats_graph=True), dict(p_grad=False),
                                dict(p_grad=False, no_grad=True), dict(no_grad=True), dict(freeze_bn=False), dict(U=20),
                                dict(arch="affine", S=1), dict(op="log_prob"), dict(op="inverse")],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_exclusions_run_what_they_run_today(kw):
    r = RT.row(**dict(dict(op="forward", D=5, rows="M", M=3, N=31, p_grad=True), **kw))
    on, today = run_row(r, True), run_row(r, None)  # today: the call as the parent commit makes it
    assert on == today and TRAIN not in on, (on, today)
    if RT.row_id(r) in RT._table():
        assert today == RT._table()[RT.row_id(r)]


def test_float64_parameters_run_what_they_run_today():
    """The grid's parameters are float32: float64 rows by hand, under the same recorders."""
    def trace_of(switch):
        torch.manual_seed(0)
        nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
        nf.context_sample_training = switch
        params = torch.zeros(3, nf.D_params, dtype=torch.float64, requires_grad=True)
        trace = []
        with RT.recording(trace), pytest.MonkeyPatch.context() as mp:
            mp.setattr(ctxsample_ops, TRAIN, lambda *a, **k: trace.append(TRAIN))
            try:
                nf._forward_from(np.zeros((3, 8, 5)), params, True)
            except RT._Reached:
                pass
        return trace

    assert trace_of(True) == trace_of(False) and trace_of(True)[-1] == "coupling"


def test_family_and_its_exclusions():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    om, p = torch.zeros(3, 8, 5), torch.zeros(3, nf.D_params, requires_grad=True)
    assert tnf.NormFlow.context_sample_training is False and nf.context_sample_training is False
    assert nf._route("forward", om, p).family == "bijectors"  # the switch defaults to off
    nf.context_rows = nf.context_training = nf.sample_training = True
    assert nf._route("forward", om, p).family == "bijectors"  # the other switches leave this cell alone
    nf.context_sample_training = True
    for others in (True, False):
        nf.context_rows = nf.context_training = nf.sample_training = others  # independent switches
        assert nf._route("forward", om, p) == ("train_context_sample", False, False)
        assert nf._route("forward", om, p, f32_draw=True) == ("train_context_sample", False, False)  # log_q: the caller's
        assert nf._route("forward", om[:, :1], p).family == "train_context_sample"
        assert nf._route("forward", torch.zeros(3, 31, 5), p).family == "train_context_sample"
        assert nf._route("forward", torch.zeros(3, 32, 5), p).family == ("train_sample" if others else "bijectors")  # N = 32
        assert nf._route("forward", om[:1], p[:1]).family == ("train_sample" if others else "bijectors")  # M_p = 1
        assert nf._route("forward", om[:1], p).family == "bijectors"  # M_z != M_p
        assert nf._route("forward", om, p, freeze_bn=False).family == "bijectors"  # fresh statistics
        assert nf._route("forward", om, p.detach()).family == ("context_rows" if others else "bijectors")  # nothing to train
        with torch.no_grad():
            assert nf._route("forward", om, p).family == ("context_rows" if others else "bijectors")
        assert nf._route("forward", om, p.double()).family == "bijectors"
        assert nf._route("forward", om.double(), p).family == "bijectors"
        assert nf._route("forward", om[0], p).family == "bijectors"  # 2-d
        assert nf._route("log_prob", om, p).family == ("train_context" if others else "bijectors")  # sampling only
        assert nf._route("inverse", om, p).family == "bijectors"
        nf.fusion = _lib.FUSE_LAYER
        assert nf._route("forward", om, p).family == "bijectors"
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("forward", om, p).family == "train_context_sample"
        nf.fusion = _lib.FUSE_AUTO
    for b in nf._bn_layers():  # statistics in the graph: only the composition differentiates through them
        b._last_mean = torch.zeros(5, requires_grad=True)
        break
    assert nf._route("forward", om, p).family == "bijectors"
    ar = tnf.NormFlow(5, True, "AR", 1, 2, 15, device="cpu")
    ar.context_sample_training = True
    assert ar._route("forward", om, torch.zeros(3, ar.D_params, requires_grad=True)).family == "bijectors"
    wide = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
    wide.context_sample_training = True
    assert wide._route("forward", om, torch.zeros(3, wide.D_params, requires_grad=True)).family == "bijectors"  # U > 16
    sup = tnf.NormFlow(5, True, "coupling", 2, 2, 15, tnf.ToInterval(5, [-1.0] * 5, [2.0] * 5), device="cpu")
    sup.context_sample_training = True
    ps = torch.zeros(3, sup.D_params, requires_grad=True)
    assert sup._route("forward", om, ps) == ("train_context_sample", False, False)  # the support layer: its own op
    d64 = tnf.NormFlow(64, True, "coupling", 4, 2, 15, device="cpu")
    d64.context_sample_training = True
    p64 = torch.zeros(3, d64.D_params, requires_grad=True)
    for n, fam in ((1, "train_context_sample"), (31, "train_context_sample"), (32, "bijectors")):
        assert d64._route("forward", torch.zeros(3, n, 64), p64).family == fam


def test_stats_walk_runs_at_most_once_per_call(monkeypatch):
    calls = []
    real = tnf.NormFlow._stats_in_graph
    monkeypatch.setattr(tnf.NormFlow, "_stats_in_graph", lambda self: (calls.append(1), real(self))[1])
    for kw in (dict(), dict(N=32), dict(rows="one", M=1), dict(stats_graph=True), dict(fusion="LAYER"), dict(D=64, N=1)):
        del calls[:]
        run_row(RT.row(**dict(dict(op="forward", D=5, rows="M", M=3, N=31, p_grad=True), **kw)), True)
        assert len(calls) <= 1, (kw, len(calls))


# ---- the algebra of the walk, before any kernel --------------------------------------------------------------------------
def check(tag, gp, go, want):
    for name, got, ref, bar in (("params", gp, want[0], BAR_P), ("omega", go, want[1], BAR_Z)):
        whole, rows = grad_err("ctxsample restatement %s %s" % (tag, name), got, ref), R.row_err(got, ref)
        print("ctxsample restatement %s %s: whole %.2e per row %.2e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


def forward32(oracle, omega, params, mean, alpha, shape):
    """The float32 z the kernel starts from: the oracle's frozen-statistics sampling pass in float32."""
    with torch.no_grad():
        return oracle.flow_forward(omega.double().numpy(), params, *shape, bn_stats=list(zip(mean, alpha)))[0]


@pytest.mark.parametrize("D,S,L,U,M,N", R.GRID, ids=lambda v: str(v))
def test_restatement_against_float64_autograd(oracle, D, S, L, U, M, N):
    """float32 gradients from a float32 z, every layer's input rebuilt by the inverse map, explicit deltas, against
    float64 autograd through the oracle's composition, over every case of tests/test_gpu_ctx_sample.py.  Measured over
    the 62 cases and the one-cotangent cases below: parameters 5.3e-7 whole and 9.8e-7 per context row, omega 3.7e-7
    both ways (the bars are BAR_P = 5e-5 and BAR_Z = 5e-6)."""
    params, mean, alpha, omega = CF.inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    shape = (D, S, L, U)
    z = forward32(oracle, omega, params, mean, alpha, shape)
    assert z.dtype == torch.float32
    gp, go, om = R.sample_bwd(z, params, mean, alpha, g_z, g_sld, *shape)
    assert gp.shape == params.shape and go.shape == omega.shape and gp.dtype == go.dtype == torch.float32
    check("D=%d S=%d L=%d U=%d M=%d N=%d" % (D, S, L, U, M, N), gp, go,
          R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape))
    torch.testing.assert_close(om, omega, rtol=1e-4, atol=1e-4)  # the walk ends at the draw (domain_helpers.INV_TOL)


@pytest.mark.parametrize("D,S,L,U,M,N", [(5, 2, 2, 15, 5, 17), (64, 1, 3, 16, 5, 31), (2, 2, 2, 15, 5, 1), (33, 2, 2, 15, 5, 2)])
def test_restatement_one_upstream_gradient_at_a_time(oracle, D, S, L, U, M, N):
    params, mean, alpha, omega = CF.inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    shape = (D, S, L, U)
    z = forward32(oracle, omega, params, mean, alpha, shape)
    for tag, a, b in (("g_z only", g_z, None), ("g_sld only", None, g_sld)):
        gp, go, _ = R.sample_bwd(z, params, mean, alpha, a, b, *shape)
        check("%s D=%d N=%d" % (tag, D, N), gp, go, R.reference(oracle, float64, omega, params, mean, alpha, a, b, shape))
    gp, go, _ = R.sample_bwd(z, params, mean, alpha, torch.zeros_like(g_z), torch.zeros_like(g_sld), *shape)
    assert not gp.any() and not go.any()  # zero upstream gradient: exactly zero everywhere
