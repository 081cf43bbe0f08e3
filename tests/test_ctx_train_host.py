"""Training per-context coupling flows with fewer than 32 samples per context in one backward launch
(include/tnf_ctxtrain.h), without a GPU: header, exports and binding table in step; the support predicate over a grid
against its definition; every refusal that precedes a launch; the routing of NormFlow with the switch `context_training`
on and off; and the algebra of the kernel's walk (tests/ctxtrain_restatement.py) against float64 autograd."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, grad_err
import ctxtrain_restatement as R
import test_gpu_ctx_flow as CF
import test_route_table as RT
from domain_helpers import BAR_P, BAR_Z, float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, ctxflow_ops, ctxtrain_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
NAMES = ("tnf_ctx_train_supported", "tnf_ctx_train_launch_count", "tnf_ctx_train_log_prob_bwd_f32")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_ctxtrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.CTXTRAIN_SIGNATURES) == sorted(NAMES) and len(protos) == 3
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES) | set(_lib.PADTRAIN_SIGNATURES) | set(_lib.PADBATCH_SIGNATURES)
              | set(_lib.CTXFLOW_SIGNATURES))
    assert not set(_lib.CTXTRAIN_SIGNATURES) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.CTXTRAIN_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.CTXTRAIN_SIGNATURES["tnf_ctx_train_launch_count"][0] is ctypes.c_int64
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_ctxtrain.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    ctxflow_h = open(os.path.join(ROOT, "include", "tnf_ctxflow.h")).read()
    assert "TNF_CTXFLOW_COUNTERS = 2" in ctxflow_h and "tnf_ctxtrain.h" in ctxflow_h
    assert _lib.DIAG_FAMILIES == 19  # a counter of its own: the flow families are a closed set
    assert lib.tnf_ctx_train_launch_count() >= 0


def test_predicate_is_its_definition_over_the_grid():
    ones = 0
    for D in range(-1, 67):
        for S in (0, 1, 4, 40):
            for L in range(0, 5):
                for U in (0, 1, 15, 16, 17):
                    for N in (0, 1, 16, 31, 32):
                        want = 2 <= D <= 64 and S >= 1 and 1 <= L <= 3 and 1 <= U <= 16 and 1 <= N <= 31
                        assert lib.tnf_ctx_train_supported(D, S, L, U, N) == int(want), (D, S, L, U, N)
                        assert lib.tnf_ctx_flow_supported(D, S, L, U, N) == int(want)  # the forward half's domain
                        assert ctxtrain_ops.ctx_train_supported(D, S, L, U, N) == want
                        ones += want
    assert ones == 63 * 3 * 3 * 3 * 3
    assert lib.tnf_ctx_train_supported(64, 1000, 3, 16, 31) == 1  # no bound on S: one layer's block at a time
    assert lib.tnf_ctx_train_supported(5, 2, 2, 15, 1 << 40) == 0 and lib.tnf_ctx_train_supported(5, 2, 2, 15, -1) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    count, counts = ctxtrain_ops.launch_count(), ctxflow_ops.launch_counts()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]
    tag = b"tnf_ctx_train_log_prob_bwd_f32"

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 15)

    def bwd(**kw):
        a = dict(z0=p[0], params=p[1], mean=p[2], alpha=p[3], g_lp=p[4], g_params=p[5], g_z=p[6], M=3, N=8, D=5, S=2, L=2,
                 U=15, pstride=P5, gpstride=P5)
        a.update(kw)
        return lib.tnf_ctx_train_log_prob_bwd_f32(a["z0"], a["params"], a["mean"], a["alpha"], a["g_lp"], a["g_params"],
                                                  a["g_z"], a["M"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                                  a["gpstride"], None)

    for name in ("z0", "params", "mean", "alpha", "g_lp", "g_params"):
        refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
    for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
        refused(bwd(**kw), INV, tag + b": M=")
    for kw in (dict(D=1), dict(D=65), dict(D=0), dict(L=4), dict(L=0), dict(U=17), dict(U=0), dict(S=0), dict(N=32),
               dict(N=1000)):
        refused(bwd(**kw), UNSUP, tag + b": no per-context kernel for D=")
    refused(bwd(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(gpstride=P5 - 1), INV, tag + b": gradient row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(pstride=0), INV, tag + b": params row has 0 elements")
    refused(bwd(g_z=p[0]), INV, tag + b": g_z must not alias z0")
    refused(bwd(g_params=p[1]), INV, tag + b": g_params must not alias params")
    assert bwd(N=0) == 0 and bwd(N=0, g_z=None) == 0  # nothing to do: OK, no launch
    refused(bwd(N=0, gpstride=P5 - 1), INV, tag + b": gradient row has")  # ... after the other checks
    assert ctxtrain_ops.launch_count() == count and ctxflow_ops.launch_counts() == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing: the method of tests/test_ctx_flow_host.py, with the new entry recorded -------------------------------------
TRAIN = "ctx_flow_log_prob_train"


def run_row(r, switch, rows_switch=None):
    """test_route_table.run_row with `NormFlow.context_training` = switch (None: the attribute absent, as on a fresh
    flow), `NormFlow.context_rows` = rows_switch, and the new entry recorded beside the two of ctxflow_ops."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is not None:
            mp.setattr(tnf.NormFlow, "context_training", switch, raising=False)
        if rows_switch is not None:
            mp.setattr(tnf.NormFlow, "context_rows", rows_switch, raising=False)
        trace = []
        for mod, name in ((ctxtrain_ops, TRAIN), (ctxflow_ops, "ctx_flow_log_prob_raw"), (ctxflow_ops, "ctx_flow_forward_raw")):
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(mod, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_context_training(r):
    """The conditions of the new row of the routing docstring, from the grid row alone.  (The grid's parameters are
    float32; a row's z has the parameters' leading dimension M.)"""
    return (r["op"] == "log_prob" and r["arch"] == "coupling" and r["zdtype"] == "float32" and not r["no_grad"]
            and (r["p_grad"] or r["z_grad"]) and not r["stats_graph"] and r["zdim"] == 3 and r["rows"] == "M" and r["M"] > 1
            and r["fusion"] != "LAYER" and lib.tnf_ctx_train_supported(r["D"], r["S"], RT.L, r["U"], r["N"]) == 1)


def test_every_row_of_the_grid_on_and_off():
    """Switch off (or absent): every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of the new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), 0
    for r in RT.GRID:
        old = table[RT.row_id(r)]
        want = takes_context_training(r)
        if not want and RT.GRID.index(r) % 5:  # every candidate row, every fifth of the others
            continue
        assert run_row(r, False) == old, RT.row_id(r)
        if want:
            assert run_row(r, None) == old, RT.row_id(r)
            assert run_row(r, False, rows_switch=True) == old, RT.row_id(r)  # context_rows alone: autograd as today
        on = run_row(r, True)
        if want and not old[-1].startswith("raises"):
            assert old[-1] in ("affine", "coupling"), RT.row_id(r)  # nothing another family takes changes hands
            assert on == old[:-1] + [TRAIN], RT.row_id(r)
            assert run_row(r, True, rows_switch=True) == on
            changed += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed >= 10, changed  # not vacuous


@pytest.mark.parametrize("kw", [dict(N=32), dict(rows="one", M=3, N=31), dict(fusion="LAYER", N=31), dict(arch="AR", S=1),
                                dict(zdtype="float64"), dict(U=20), dict(stats_graph=True), dict(zdim=2),
                                dict(p_grad=False, no_grad=True), dict(p_grad=False), dict(arch="affine", S=1)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_exclusions_run_what_they_run_today(kw):
    r = RT.row(**dict(dict(op="log_prob", D=5, rows="M", M=3, N=31, p_grad=True), **kw))
    on = run_row(r, True)
    with pytest.MonkeyPatch.context() as mp:  # today: the call as the parent commit makes it
        mp.delattr(tnf.NormFlow, "context_training", raising=False)
        today = RT.run_row(r)
    assert on == today and TRAIN not in on, (on, today)
    if RT.row_id(r) in RT._table():
        assert today == RT._table()[RT.row_id(r)]


def test_family_and_its_exclusions():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    P = nf.D_params
    z, p = torch.zeros(3, 8, 5), torch.zeros(3, P, requires_grad=True)
    zg = torch.zeros(3, 8, 5, requires_grad=True)
    assert getattr(nf, "context_training", False) is False
    assert nf._route("log_prob", z, p).family == "bijectors"  # the switch defaults to off
    nf.context_rows = True
    assert nf._route("log_prob", z, p).family == "bijectors"  # context_rows alone leaves autograd calls alone
    nf.context_training = True
    for rows in (True, False):
        nf.context_rows = rows  # independent switches
        assert nf._route("log_prob", z, p) == ("train_context", False, False)
        assert nf._route("log_prob", zg, p.detach()).family == "train_context"  # only z requires grad
        assert nf._route("log_prob", zg, p).family == "train_context"
        assert nf._route("log_prob", z[:1], p).family == "train_context"  # one shared block that needs no gradient
        assert nf._route("log_prob", zg[:1], p).family == "bijectors"  # ... its gradient would sum over contexts
        assert nf._route("log_prob", torch.zeros(2, 8, 5), p).family == "bijectors"  # M_z not in {1, M}
        assert nf._route("log_prob", torch.zeros(3, 32, 5), p).family == "bijectors"  # N = 32
        assert nf._route("log_prob", z, p[:1]).family != "train_context"  # one shared row
        assert nf._route("log_prob", z.double(), p).family == "bijectors"
        assert nf._route("log_prob", z, p.double()).family == "bijectors"
        assert nf._route("log_prob", z[0], p).family == "bijectors"  # 2-d z
        assert nf._route("inverse", z, p).family == "bijectors"  # log_prob only
        assert nf._route("forward", z, p).family == "bijectors"
        assert nf._route("log_prob", z, p.detach()).family == ("context_rows" if rows else "bijectors")  # nothing to train
        with torch.no_grad():
            assert nf._route("log_prob", z, p).family == ("context_rows" if rows else "bijectors")
        nf.fusion = _lib.FUSE_LAYER
        assert nf._route("log_prob", z, p).family == "bijectors"
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("log_prob", z, p).family == "train_context"
        nf.fusion = _lib.FUSE_AUTO
    for b in nf._bn_layers():  # statistics in the graph: only the composition differentiates through them
        b._last_mean = torch.zeros(5, requires_grad=True)
        break
    assert nf._route("log_prob", z, p).family == "bijectors"
    ar = tnf.NormFlow(5, True, "AR", 1, 2, 15, device="cpu")
    ar.context_training = True
    assert ar._route("log_prob", z, torch.zeros(3, ar.D_params, requires_grad=True)).family != "train_context"
    wide = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
    wide.context_training = True
    assert wide._route("log_prob", z, torch.zeros(3, wide.D_params, requires_grad=True)).family == "bijectors"  # U > 16
    sup = tnf.NormFlow(5, True, "coupling", 2, 2, 15, tnf.ToInterval(5, [-1.0] * 5, [2.0] * 5), device="cpu")
    sup.context_training = True
    ps = torch.zeros(3, sup.D_params, requires_grad=True)
    assert sup._route("log_prob", z, ps) == ("train_context", False, False)  # the support layer: its own kernel
    assert sup._route("inverse", z, ps).family == "bijectors"
    d64 = tnf.NormFlow(64, True, "coupling", 4, 2, 15, device="cpu")
    d64.context_training = True
    p64 = torch.zeros(3, d64.D_params, requires_grad=True)
    for n, fam in ((1, "train_context"), (31, "train_context"), (32, "train_reversible")):
        assert d64._route("log_prob", torch.zeros(3, n, 64), p64).family == fam


# ---- the algebra of the walk, before any kernel --------------------------------------------------------------------------
def row_err(got, want):
    """The largest error of a context's row relative to that row's largest entry, over the contexts."""
    got, want = got.detach().double().flatten(1), want.detach().double().flatten(1)
    return float(((got - want).abs().max(1).values / want.abs().max(1).values.clamp_min(1e-300)).max())


@pytest.mark.parametrize("D,S,L,U,M,N", [(5, 2, 2, 15, 5, 8), (2, 1, 1, 15, 5, 1), (33, 2, 3, 16, 5, 17), (64, 4, 2, 15, 4, 31)])
def test_restatement_against_float64_autograd(oracle, D, S, L, U, M, N):
    """float32 gradients rebuilt from a float32 z0, explicit deltas, rows beyond N with zero upstream gradient, against
    float64 autograd through the oracle: measured within 7.5e-7 (parameters) and 4.4e-7 (z) per context row."""
    params, mean, alpha, z = CF.inputs(oracle, D, S, L, U, M, N)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(7))
    with float64():
        p64, z64 = params.double().requires_grad_(), z.double().requires_grad_()
        (oracle.flow_log_prob(z64, p64, D, S, L, U, CF.st64(mean, alpha)) * g.double()).sum().backward()
    with torch.no_grad():
        z0, _ = oracle.flow_inverse(z, params, D, S, L, U, list(zip(mean, alpha)))
        gp0, gz0 = R.log_prob_bwd(z0, params, mean, alpha, g, D, S, L, U, pad_to=0)
        gp, gz = R.log_prob_bwd(z0, params, mean, alpha, g, D, S, L, U, pad_to=16)
    assert gp.shape == params.shape and gz.shape == z.shape
    for name, got, want, bar in (("params", gp, p64.grad, BAR_P), ("z", gz, z64.grad, BAR_Z)):
        tag = "ctxtrain restatement %s D=%d N=%d" % (name, D, N)
        print(tag, "whole %.2e per row %.2e" % (grad_err(tag, got, want), row_err(got, want)))
        grad_err(tag, got, want, bar)
        assert row_err(got, want) <= bar
    # rows beyond N with zero upstream gradient contribute exactly nothing: all their deltas are +-0, and the result is
    # that of the N rows alone up to the row blocking of the CPU matmuls of the recomputed forward
    assert R.PAD_ABS[0] == 0.0
    assert grad_err("ctxtrain restatement pad params", gp, gp0) <= 2e-6 and grad_err("ctxtrain restatement pad z", gz, gz0) <= 2e-6
    # zero upstream gradient: exactly zero everywhere
    gpz, gzz = R.log_prob_bwd(z0, params, mean, alpha, torch.zeros(M, N), D, S, L, U)
    assert not gpz.any() and not gzz.any()
