"""Per-context coupling flows with fewer than 32 samples per context in one launch (include/tnf_ctxflow.h), without a
GPU: header, exports and binding table in step; the support predicate over a grid against its definition; every refusal
that precedes a launch; and the routing of NormFlow with the switch `context_rows` on and off."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import test_route_table as RT

import torch_nf_amd as tnf
from torch_nf_amd import _lib, ctxflow_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
COUNTERS = ("LOG_PROB", "FORWARD")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_ctxflow.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.CTXFLOW_SIGNATURES) and len(protos) == 4
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES) | set(_lib.PADTRAIN_SIGNATURES) | set(_lib.PADBATCH_SIGNATURES))
    assert not set(_lib.CTXFLOW_SIGNATURES) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.CTXFLOW_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.CTXFLOW_SIGNATURES["tnf_ctx_flow_launch_count"][0] is ctypes.c_int64
    header = open(os.path.join(ROOT, "include", "tnf_ctxflow.h")).read()
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_ctxflow.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    for i, n in enumerate(COUNTERS):
        assert "TNF_CTXFLOW_COUNT_%s = %d" % (n, i) in header
    assert "TNF_CTXFLOW_COUNTERS = 2" in header
    assert (ctxflow_ops.COUNT_LOG_PROB, ctxflow_ops.COUNT_FORWARD) == (0, 1)
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(2):
        assert lib.tnf_ctx_flow_launch_count(which) >= 0
    assert lib.tnf_ctx_flow_launch_count(2) == -1 and b"tnf_ctx_flow_launch_count" in lib.tnf_last_error()
    assert lib.tnf_ctx_flow_launch_count(-1) == -1


def test_predicate_is_its_definition_over_the_grid():
    ones = 0
    for D in range(-1, 67):
        for S in (0, 1, 4, 40):
            for L in range(0, 5):
                for U in (0, 1, 15, 16, 17):
                    for N in (0, 1, 16, 31, 32):
                        want = 2 <= D <= 64 and S >= 1 and 1 <= L <= 3 and 1 <= U <= 16 and 1 <= N <= 31
                        assert lib.tnf_ctx_flow_supported(D, S, L, U, N) == int(want), (D, S, L, U, N)
                        assert ctxflow_ops.ctx_flow_supported(D, S, L, U, N) == want
                        ones += want
    assert ones == 63 * 3 * 3 * 3 * 3
    assert lib.tnf_ctx_flow_supported(64, 1000, 3, 16, 31) == 1  # no bound on S: operands live one layer at a time
    assert lib.tnf_ctx_flow_supported(5, 2, 2, 15, 1 << 40) == 0 and lib.tnf_ctx_flow_supported(5, 2, 2, 15, -1) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    counts = ctxflow_ops.launch_counts()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 15)

    def log_prob(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], lp=p[4], z0=p[5], sld=p[6], Mz=3, M=3, N=8, D=5, S=2, L=2, U=15,
                 pstride=P5)
        a.update(kw)
        return lib.tnf_ctx_flow_log_prob_f32(a["z"], a["params"], a["mean"], a["alpha"], a["lp"], a["z0"], a["sld"],
                                             a["Mz"], a["M"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    def forward(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], z0=p[5], sld=p[6], M=3, N=8, D=5, S=2, L=2, U=15, pstride=P5)
        a.update(kw)
        return lib.tnf_ctx_flow_forward_f32(a["z"], a["params"], a["mean"], a["alpha"], a["z0"], a["sld"], a["M"], a["N"],
                                            a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    unsupported = (dict(D=1), dict(D=65), dict(D=0), dict(L=4), dict(L=0), dict(U=17), dict(U=0), dict(S=0), dict(N=32),
                   dict(N=1000))
    for call, tag in ((log_prob, b"tnf_ctx_flow_log_prob_f32"), (forward, b"tnf_ctx_flow_forward_f32")):
        for name in ("z", "params", "mean", "alpha"):
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
            refused(call(**kw), INV, tag + b": M_z=")
        for kw in unsupported:
            refused(call(**kw), UNSUP, tag + b": no per-context kernel for D=")
        refused(call(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
        assert call(N=0) == 0  # nothing to do: OK, no launch
        refused(call(N=0, pstride=P5 - 1), INV, tag + b": params row has")  # ... after the other checks
    refused(log_prob(lp=None, z0=None, sld=None), INV, b"tnf_ctx_flow_log_prob_f32: no output requested")
    refused(forward(z0=None, sld=None), INV, b"tnf_ctx_flow_forward_f32: no output requested")
    for kw in (dict(Mz=2), dict(Mz=0), dict(Mz=4)):
        refused(log_prob(**kw), INV, b"tnf_ctx_flow_log_prob_f32: M_z=%d M=3" % kw["Mz"])
    refused(log_prob(z0=p[0]), INV, b"z0 must not alias z")
    refused(forward(z0=p[0]), INV, b"z_out must not alias omega")
    assert log_prob(Mz=1, N=0) == 0 and log_prob(lp=None, sld=None, N=0) == 0 and forward(sld=None, N=0) == 0
    assert ctxflow_ops.launch_counts() == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing: the method of tests/test_route_table.py, with the new entries recorded too ---------------------------------
LP, FWD = "ctx_flow_log_prob_raw", "ctx_flow_forward_raw"


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.context_rows` = switch (None: the attribute absent, as on a fresh flow)
    and the two new entries recorded."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is not None:
            mp.setattr(tnf.NormFlow, "context_rows", switch, raising=False)
        trace = []
        for name in (LP, FWD):
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(ctxflow_ops, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_context_rows(r):
    """The conditions of the new row of the routing docstring, from the grid row alone -> LP, FWD or None.  (The grid's
    parameters are float32; omega is drawn with the parameters' leading dimension, float32 on the device whatever
    `zdtype` and `z_grad` say.)"""
    forward = r["op"] == "forward"
    if not (r["arch"] == "coupling" and (r["freeze_bn"] or not forward) and r["fusion"] != "LAYER" and r["rows"] == "M"
            and r["M"] > 1 and (forward or r["zdim"] == 3) and not (r["sup"] and r["op"] == "inverse")
            and lib.tnf_ctx_flow_supported(r["D"], r["S"], RT.L, r["U"], r["N"]) == 1):
        return None
    if not forward and r["zdtype"] != "float32":
        return None
    if not forward and r["D"] == 64 and r["N"] <= 5:
        return None  # the one measured exception: the composition is faster there
    plain = r["no_grad"] or not (r["p_grad"] or (r["z_grad"] and not forward))
    if not plain or (r["stats_graph"] and not r["no_grad"]):
        return None
    return FWD if forward else LP


def test_family_with_the_switch_on():
    for D in (5, 32, 33, 48, 64):  # the widths whose per-context rows the recorded table holds
        for op, entry in (("log_prob", LP), ("inverse", LP), ("forward", FWD)):
            for shape in (dict(M=3, N=31), dict(M=4, N=1)):
                r = RT.row(op=op, D=D, rows="M", no_grad=True, **shape)
                old = RT._table()[RT.row_id(r)]  # the rows the recorded table pins: the per-bijector composition
                assert old[-1] in ("affine", "coupling")
                if D == 64 and op != "forward" and shape["N"] <= 5:
                    entry = old[-1]  # slower than the composition there: left to it
                assert run_row(r, True) == old[:-1] + [entry], (D, op, shape)
                assert run_row(r, False) == old == run_row(r, None)
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    nf.context_rows = True
    P = nf.D_params
    with torch.no_grad():
        assert nf._route("log_prob", torch.zeros(3, 8, 5), torch.zeros(3, P)).family == "context_rows"
        assert nf._route("log_prob", torch.zeros(1, 8, 5), torch.zeros(3, P)).family == "context_rows"  # one block of z
        assert nf._route("inverse", torch.zeros(3, 8, 5), torch.zeros(3, P)).family == "context_rows"
        assert nf._route("forward", torch.zeros(3, 8, 5), torch.zeros(3, P)) == ("context_rows", False, False)
        assert nf._route("forward", torch.zeros(3, 8, 5), torch.zeros(3, P), f32_draw=True) == ("context_rows", False, False)
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("log_prob", torch.zeros(3, 8, 5), torch.zeros(3, P)).family == "context_rows"
    # nothing requires grad with grad mode on: plain
    assert nf._route("log_prob", torch.zeros(3, 8, 5), torch.zeros(3, P)).family == "context_rows"


def test_exclusions_take_todays_route():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    nf.context_rows = True
    P = nf.D_params
    z, p = torch.zeros(3, 8, 5), torch.zeros(3, P)
    with torch.no_grad():
        assert nf._route("log_prob", z, p).family == "context_rows"
        assert nf._route("log_prob", torch.zeros(3, 32, 5), p).family == "padded"  # N = 32
        assert nf._route("log_prob", z, p[:1]).family == "padded"  # one shared row
        assert nf._route("log_prob", torch.zeros(2, 8, 5), p).family == "bijectors"  # M_z not in {1, M}
        assert nf._route("forward", torch.zeros(1, 8, 5), p).family == "bijectors"  # sampling: one block per context
        assert nf._route("forward", z, p, freeze_bn=False).family == "bijectors"  # fresh statistics
        assert nf._route("log_prob", z.double(), p).family == "bijectors"
        assert nf._route("log_prob", z, p.double()).family == "bijectors"
        assert nf._route("log_prob", z[0], p).family == "bijectors"  # 2-d z
        nf.fusion = _lib.FUSE_LAYER
        assert nf._route("log_prob", z, p).family == "bijectors"
        nf.fusion = _lib.FUSE_AUTO
        d64 = tnf.NormFlow(64, True, "coupling", 4, 2, 15, device="cpu")
        d64.context_rows = True
        p64 = torch.zeros(3, d64.D_params)
        for n, fam in ((1, "bijectors"), (5, "bijectors"), (6, "context_rows"), (31, "context_rows")):
            assert d64._route("log_prob", torch.zeros(3, n, 64), p64).family == fam  # the measured break-even
            assert d64._route("inverse", torch.zeros(3, n, 64), p64).family == fam
            assert d64._route("forward", torch.zeros(3, n, 64), p64).family == "context_rows"
        nf.context_rows = False
        assert nf._route("log_prob", z, p).family == "bijectors"
        nf.context_rows = True
    pg = p.clone().requires_grad_()
    assert nf._route("log_prob", z, pg).family == "bijectors"  # autograd keeps today's routes
    assert nf._route("log_prob", z.clone().requires_grad_(), p).family == "bijectors"
    with torch.no_grad():
        assert nf._route("log_prob", z, pg).family == "context_rows"
        ar = tnf.NormFlow(5, True, "AR", 1, 2, 15, device="cpu")
        ar.context_rows = True
        assert ar._route("log_prob", z, torch.zeros(3, ar.D_params)).family == "ar_fused"
        wide = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
        wide.context_rows = True
        assert wide._route("log_prob", z, torch.zeros(3, wide.D_params)).family == "bijectors"  # num_units > 16
        sup = tnf.NormFlow(5, True, "coupling", 2, 2, 15, tnf.ToInterval(5, [-1.0] * 5, [2.0] * 5), device="cpu")
        sup.context_rows = True
        ps = torch.zeros(3, sup.D_params)
        assert sup._route("log_prob", z, ps) == ("context_rows", False, False)  # the support layer: its own kernel
        assert sup._route("forward", z, ps) == ("context_rows", False, False)
        assert sup._route("inverse", z, ps).family == "bijectors"


@pytest.mark.parametrize("kw", [dict(p_grad=True), dict(N=32), dict(rows="one", M=3, N=31), dict(fusion="LAYER", N=31),
                                dict(arch="AR", S=1), dict(zdtype="float64"), dict(U=20), dict(stats_graph=True),
                                dict(arch="affine", S=1)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
@pytest.mark.parametrize("op", ["log_prob", "inverse", "forward"])
def test_exclusions_run_what_they_run_today(kw, op):
    base = dict(op=op, D=5, rows="M", M=3, N=31)
    if "p_grad" not in kw and "stats_graph" not in kw:
        base["no_grad"] = True
    r = RT.row(**dict(base, **kw))
    on = run_row(r, True)
    with pytest.MonkeyPatch.context() as mp:  # today: the call as the parent commit makes it
        mp.delattr(tnf.NormFlow, "context_rows", raising=False)
        today = RT.run_row(r)
    if kw == dict(zdtype="float64") and op == "forward":
        return  # the grid draws omega in float32 whatever zdtype says: not an exclusion for sampling
    assert on == today and LP not in on and FWD not in on, (on, today)
    if RT.row_id(r) in RT._table():
        assert today == RT._table()[RT.row_id(r)]


def test_every_row_of_the_grid_on_and_off():
    """Switch off (or absent): every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of the new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), {LP: 0, FWD: 0}
    for r in RT.GRID:
        old = table[RT.row_id(r)]
        want = takes_context_rows(r)
        if want is None and RT.GRID.index(r) % 5:  # every candidate row, every fifth of the others
            continue
        assert run_row(r, False) == old, RT.row_id(r)
        on = run_row(r, True)
        if want is not None and not old[-1].startswith("raises"):
            assert old[-1] in ("affine", "coupling"), RT.row_id(r)  # nothing another family takes changes hands
            assert on == old[:-1] + [want], RT.row_id(r)
            changed[want] += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed[LP] >= 10 and changed[FWD] >= 10, changed  # not vacuous


def test_switch_defaults_to_off():
    nf = tnf.NormFlow(4, True, "coupling", 1, 1, 15, device="cpu")
    assert getattr(nf, "context_rows", False) is False
    with torch.no_grad():
        assert nf._route("log_prob", torch.zeros(8, 4, 4), torch.zeros(8, nf.D_params)).family == "bijectors"
        nf.context_rows = True
        assert nf._route("log_prob", torch.zeros(8, 4, 4), torch.zeros(8, nf.D_params)).family == "context_rows"
