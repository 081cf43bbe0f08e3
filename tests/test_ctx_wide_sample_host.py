"""Training per-context coupling flows with 17 .. 64 units and fewer than 32 draws per context through their
frozen-statistics samples in one backward launch (include/tnf_ctxwidesample.h, csrc/flow_ctx_wide_sample_bwd.hip,
NormFlow's family `train_context_sample_wide`), without a GPU: header, exports and binding table in step; the support
predicate and the team-size rule against their restated definitions; every refusal that precedes a launch; the routing of
NormFlow with the switch `wide_context_sample_training` on, off and absent; and the algebra of the walk
(tests/ctxsample_restatement.py, width-agnostic) from a float32 z against float64 autograd over the cases of the GPU
test (tests/ctxwidesample_restatement.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import ctxwide_restatement as W
import ctxwidesample_restatement as R
import test_gpu_ctx_flow as CF
import test_route_table as RT
from domain_helpers import BAR_P, BAR_Z, float64

import torch_nf_amd as tnf
from torch_nf_amd import (_lib, ctxflow_ops, ctxsample_ops, ctxtrain_ops, ctxwide_ops, ctxwidesample_ops, wideflow_ops)

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
HEADER = os.path.join(ROOT, "include", "tnf_ctxwidesample.h")
NAMES = ("tnf_ctx_wide_sample_supported", "tnf_ctx_wide_sample_launch_count", "tnf_ctx_wide_sample_waves",
         "tnf_ctx_wide_sample_set_waves", "tnf_ctx_wide_sample_bwd_f32")
TABLE = "CTXWIDESAMPLE_ENTRIES"


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    table = getattr(_lib, TABLE)
    assert sorted(protos) == sorted(table) == sorted(NAMES) and len(protos) == 5
    assert not TABLE.endswith("SIGNATURES")  # the `*SIGNATURES` tables are a closed set of fifteen
    others = [n for n in dir(_lib) if n.endswith("SIGNATURES")]
    assert len(others) == 15
    for n in others:
        assert not set(table) & set(getattr(_lib, n)), n  # disjoint from every other table
    assert len(_lib.CTXWIDE_SIGNATURES) == 7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = table[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert table["tnf_ctx_wide_sample_launch_count"][0] is ctypes.c_int64
    # the arguments are exactly those of the 16-unit entry
    assert table["tnf_ctx_wide_sample_bwd_f32"] == _lib.CTXSAMPLE_SIGNATURES["tnf_ctx_sample_bwd_f32"]
    assert table["tnf_ctx_wide_sample_supported"] == _lib.CTXSAMPLE_SIGNATURES["tnf_ctx_sample_supported"]
    old = _declared(os.path.join(ROOT, "include", "tnf_ctxsample.h"))["tnf_ctx_sample_bwd_f32"]
    assert [re.sub(r"\s+", " ", p).strip() for p in protos["tnf_ctx_wide_sample_bwd_f32"]] == \
        [re.sub(r"\s+", " ", p).strip() for p in old]
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_ctxwidesample.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    assert _lib.DIAG_FAMILIES == 19  # a counter of its own: the flow families are a closed set
    assert "TNF_CTXWIDE_COUNTERS = 3" in open(os.path.join(ROOT, "include", "tnf_ctxwide.h")).read()
    assert lib.tnf_ctx_wide_sample_launch_count() >= 0
    makefile = open(os.path.join(ROOT, "torch_nf_amd", "csrc", "Makefile")).read()
    for word in ("flow_ctx_wide_sample_bwd.hip", "ctx_sample_step.h", "../../include/tnf_ctxwidesample.h"):
        assert word in makefile, word


def test_predicate_is_the_conjunction_over_the_domain():
    """D 1 .. 65, L 0 .. 6, U 15 .. 65, N in {0, 1, 16, 31, 32}, S in {0, 1, 9}: the predicate is the forward's and the
    backward's, both, as restated by tests/ctxwide_restatement.py; the existing predicates keep their values."""
    ones = 0
    for D in range(1, 66):
        for L in range(0, 7):
            for U in range(15, 66):
                for N in (0, 1, 16, 31, 32):
                    for S in (0, 1, 9):
                        a = (D, S, L, U, N)
                        fwd, trn = W.ctx_wide_supported(*a), W.ctx_wide_train_supported(*a)
                        assert lib.tnf_ctx_wide_sample_supported(*a) == int(fwd and trn) == int(R.sample_supported(*a)), a
                        assert lib.tnf_ctx_wide_supported(*a) == int(fwd) and lib.tnf_ctx_wide_train_supported(*a) == int(trn)
                        ones += fwd and trn
                        if U <= 17:
                            narrow = 2 <= D <= 64 and S >= 1 and 1 <= L <= 3 and 1 <= U <= 16 and 1 <= N <= 31
                            assert lib.tnf_ctx_sample_supported(*a) == int(narrow), a
                            assert not (narrow and fwd and trn)  # the unit ranges are disjoint: nothing changes hands
    assert ones > 40000, ones
    assert ctxwidesample_ops.ctx_wide_sample_supported(5, 2, 2, 20, 8)
    assert not ctxwidesample_ops.ctx_wide_sample_supported(5, 2, 2, 16, 8)
    assert not ctxwidesample_ops.ctx_wide_sample_supported(5, 2, 2, 20, 32)
    assert not ctxwidesample_ops.ctx_wide_sample_supported(5, 2, 4, 20, 8)  # the backward's depth
    assert R.sample_supported(64, 1, 3, 64, 22) and not R.sample_supported(64, 1, 3, 64, 23)  # ... and its slice
    assert lib.tnf_ctx_wide_sample_supported(64, 1 << 30, 2, 64, 31) == 1  # no bound on S
    assert lib.tnf_ctx_wide_sample_supported(5, 2, 2, 20, 1 << 40) == 0
    for c in R.GRID + R.ONE_COTANGENT:
        assert R.sample_supported(*c[:4], c[5]), c
    assert W.lds_bytes(W.BWD, 64, 1, 2, 64, 31) == 123008 and W.lds_bytes(W.BWD, 33, 1, 3, 64, 31) == 144512


def test_team_size_rule_and_override():
    seen = set()
    for D in range(1, 66):
        for U in range(15, 66):
            for N in (0, 1, 8, 16, 17, 31, 32):
                got = lib.tnf_ctx_wide_sample_waves(D, U, N)
                assert got == R.auto_waves(D, U, N) == ctxwidesample_ops.waves(D, U, N), (D, U, N)
                assert (got == -1) == (not W.in_domain(D, 1, U, N)) and got in (-1,) + R.TEAM_SIZES
                seen.add(got)
    assert seen == {-1, 4, 8, 16}
    assert {R.auto_waves(c[0], c[3], c[5]) for c in R.GRID} == set(R.TEAM_SIZES)  # the GPU test's cases reach all three
    assert ctxwidesample_ops.TEAMS == R.TEAM_SIZES
    count = ctxwidesample_ops.launch_count()
    first = lib.tnf_ctx_wide_sample_set_waves(0)
    try:
        assert first == 0  # automatic is the default
        for bad in (1, 2, 3, 32, -1, 5, 64):
            assert lib.tnf_ctx_wide_sample_set_waves(bad) == INV
            assert b"tnf_ctx_wide_sample_set_waves" in lib.tnf_last_error()
            with pytest.raises(_lib.TnfError):
                ctxwidesample_ops.set_waves(bad)
        prev = 0
        for w in (4, 8, 16, 0, 16, 4, 0):
            assert ctxwidesample_ops.set_waves(w) == prev  # the previous value; a refused one changed nothing
            prev = w
        assert lib.tnf_ctx_wide_sample_set_waves(7) == INV and ctxwidesample_ops.set_waves(0) == 0
        # the override changes the launch, never the automatic rule's answer
        ctxwidesample_ops.set_waves(16)
        assert lib.tnf_ctx_wide_sample_waves(4, 20, 1) == 4
    finally:
        lib.tnf_ctx_wide_sample_set_waves(0)
    assert ctxwidesample_ops.launch_count() == count


# ---- refusals --------------------------------------------------------------------------------------------------------
def _others():
    return (ctxflow_ops.launch_counts(), ctxtrain_ops.launch_count(), ctxsample_ops.launch_count(),
            wideflow_ops.launch_counts(), ctxwide_ops.launch_counts(),
            [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)])


def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    count, others = ctxwidesample_ops.launch_count(), _others()
    tag = b"tnf_ctx_wide_sample_bwd_f32"

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 20)

    def bwd(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], g_z=p[4], g_sld=p[5], g_params=p[6], g_omega=p[7], M=3, N=8,
                 D=5, S=2, L=2, U=20, pstride=P5, gpstride=P5)
        a.update(kw)
        return lib.tnf_ctx_wide_sample_bwd_f32(a["z"], a["params"], a["mean"], a["alpha"], a["g_z"], a["g_sld"],
                                               a["g_params"], a["g_omega"], a["M"], a["N"], a["D"], a["S"], a["L"], a["U"],
                                               a["pstride"], a["gpstride"], None)

    for name in ("z", "params", "mean", "alpha", "g_params"):
        refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
    refused(bwd(g_z=None, g_sld=None), INV, tag + b": no upstream gradient")
    refused(bwd(g_z=None, g_sld=None, g_omega=None), INV, tag + b": no upstream gradient")
    refused(bwd(g_z=None, g_sld=None, M=0), INV, tag + b": no upstream gradient")  # the 16-unit entry's order
    for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
        refused(bwd(**kw), INV, tag + b": M=")
    refused(bwd(M=32768 * 65535 + 1), INV, tag + b": M=2147450881 exceeds the grid")
    refused(bwd(M=0, D=1), INV, tag + b": M=")  # the shape comes after the counts
    for kw in (dict(D=1), dict(D=65), dict(D=0), dict(L=0), dict(L=4), dict(U=16), dict(U=15), dict(U=65), dict(U=0),
               dict(S=0), dict(N=32), dict(N=1000), dict(D=64, L=3, U=64, N=23), dict(D=64, L=3, U=64, N=31)):
        refused(bwd(**kw), UNSUP, tag + b": no wide per-context sampling backward for D=")
    refused(bwd(D=1, pstride=0), UNSUP, tag + b": no wide per-context")  # ... and before the strides
    refused(bwd(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(gpstride=P5 - 1), INV, tag + b": gradient row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(pstride=0), INV, tag + b": params row has 0 elements")
    refused(bwd(pstride=0, g_omega=p[0]), INV, tag + b": params row has 0 elements")  # the strides before the aliasing
    refused(bwd(g_omega=p[0]), INV, tag + b": g_omega must not alias z or g_z")
    refused(bwd(g_omega=p[4]), INV, tag + b": g_omega must not alias z or g_z")
    refused(bwd(g_params=p[1]), INV, tag + b": g_params must not alias params")
    assert bwd(N=0) == 0 and bwd(N=0, g_omega=None) == 0 and bwd(N=0, g_z=None) == 0  # nothing to do: OK, no launch
    refused(bwd(N=0, gpstride=P5 - 1), INV, tag + b": gradient row has")  # ... after the other checks
    refused(bwd(N=0, g_params=p[1]), INV, tag + b": g_params must not alias params")
    refused(bwd(N=0, L=4), UNSUP, tag + b": no wide per-context")
    assert ctxwidesample_ops.launch_count() == count and _others() == others  # nothing was launched


# ---- routing: the method of tests/test_ctx_sample_host.py, with the new entry recorded -----------------------------------
TRAIN = "ctx_wide_sample_train"
SWITCH = "wide_context_sample_training"
RELATED = ("context_rows", "context_training", "context_sample_training", "sample_training", "wide_context_rows",
           "wide_context_training")  # the six related switches
RECORDED = ((ctxwidesample_ops, TRAIN), (ctxsample_ops, "ctx_flow_sample_train"),
            (ctxtrain_ops, "ctx_flow_log_prob_train"), (ctxwide_ops, "ctx_wide_log_prob_train"),
            (ctxflow_ops, "ctx_flow_log_prob_raw"), (ctxflow_ops, "ctx_flow_forward_raw"),
            (ctxwide_ops, "ctx_wide_log_prob_raw"), (ctxwide_ops, "ctx_wide_forward_raw"))


def run_row(r, switch, others=None):
    """test_route_table.run_row with `NormFlow.wide_context_sample_training` = switch (None: the attribute absent, as on
    the parent commit), the six related switches = others (None: as they are), and the entries of the per-context
    families recorded."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is None:
            mp.delattr(tnf.NormFlow, SWITCH, raising=False)
        else:
            mp.setattr(tnf.NormFlow, SWITCH, switch, raising=False)
        if others is not None:
            for name in RELATED:
                mp.setattr(tnf.NormFlow, name, others, raising=False)
        trace = []
        for mod, name in RECORDED:
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(mod, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_the_new_family(r):
    """The conditions of the new row of the routing docstring, from the grid row alone."""
    return (r["op"] == "forward" and r["freeze_bn"] and r["arch"] == "coupling" and not r["no_grad"] and r["p_grad"]
            and not r["stats_graph"] and r["rows"] == "M" and r["M"] > 1 and r["fusion"] != "LAYER"
            and lib.tnf_ctx_wide_sample_supported(r["D"], r["S"], RT.L, r["U"], r["N"]) == 1)


def test_every_row_of_the_grid_on_off_and_absent():
    """Switch off or absent: every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of the new family hold, and then only in its last entry -- the kernel entry that the call reaches.  (The
    recorded grid has no 20-unit row with several parameter rows: rows of that kind follow by hand.)"""
    table = RT._table()
    for i, r in enumerate(RT.GRID):
        old = table[RT.row_id(r)]
        want = takes_the_new_family(r)
        on = run_row(r, True)
        if want:
            assert old[-1] == "coupling", RT.row_id(r)  # nothing another family takes changes hands
            assert on == old[:-1] + [TRAIN], RT.row_id(r)
        else:
            assert on == old, RT.row_id(r)
        if want or r["U"] == 20 or not i % 7:  # off and absent: every candidate, every 20-unit row, each seventh other
            assert run_row(r, False) == old, RT.row_id(r)
            assert run_row(r, None) == old, RT.row_id(r)
    changed = 0
    for U in (17, 20, 64):
        for D in (2, 5, 33, 64):
            for N in (1, 8, 31):
                for fusion in ("AUTO", "FLOW"):
                    r = RT.row(op="forward", D=D, U=U, S=2, rows="M", M=3, N=N, p_grad=True, fusion=fusion)
                    assert takes_the_new_family(r)
                    old = run_row(r, None)
                    assert old[-1] == "coupling" and run_row(r, False) == old
                    on = run_row(r, True)
                    assert on == old[:-1] + [TRAIN], RT.row_id(r)
                    if D == 5:
                        assert run_row(r, True, others=True) == on  # independent of the six related switches
                        assert run_row(r, True, others=False) == on
                    changed += 1
    assert changed == 72


@pytest.mark.parametrize("kw", [dict(rows="one", M=1, N=31), dict(rows="one", M=3, N=31), dict(N=32), dict(N=64),
                                dict(arch="AR", S=1), dict(fusion="LAYER"), dict(stats_graph=True), dict(p_grad=False),
                                dict(p_grad=False, no_grad=True), dict(no_grad=True), dict(freeze_bn=False), dict(U=16),
                                dict(U=15), dict(arch="affine", S=1, U=15), dict(op="log_prob"), dict(op="inverse")],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_exclusions_run_what_they_run_today(kw):
    r = RT.row(**dict(dict(op="forward", D=5, U=20, S=2, rows="M", M=3, N=31, p_grad=True), **kw))
    on, today = run_row(r, True), run_row(r, None)  # today: the call as the parent commit makes it
    assert on == today and TRAIN not in on, (on, today)
    if RT.row_id(r) in RT._table():
        assert today == RT._table()[RT.row_id(r)]


def test_float64_parameters_run_what_they_run_today():
    """The grid's parameters are float32: float64 rows by hand, under the same recorders."""
    def trace_of(switch):
        torch.manual_seed(0)
        nf = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
        nf.wide_context_sample_training = switch
        params = torch.zeros(3, nf.D_params, dtype=torch.float64, requires_grad=True)
        trace = []
        with RT.recording(trace), pytest.MonkeyPatch.context() as mp:
            mp.setattr(ctxwidesample_ops, TRAIN, lambda *a, **k: trace.append(TRAIN))
            try:
                nf._forward_from(np.zeros((3, 8, 5)), params, True)
            except RT._Reached:
                pass
        return trace

    assert trace_of(True) == trace_of(False) and trace_of(True)[-1] == "coupling"


def test_family_and_its_exclusions():
    FAM = "train_context_sample_wide"
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 20, device="cpu")
    om, p = torch.zeros(3, 8, 5), torch.zeros(3, nf.D_params, requires_grad=True)
    assert tnf.NormFlow.wide_context_sample_training is False and nf.wide_context_sample_training is False
    assert SWITCH not in vars(nf)  # a class attribute: an instance made before the switch existed behaves the same
    assert nf._route("forward", om, p).family == "bijectors"  # the switch defaults to off
    for name in RELATED:
        setattr(nf, name, True)
    assert nf._route("forward", om, p).family == "bijectors"  # the other switches leave this cell alone
    nf.wide_context_sample_training = True
    for others in (True, False):
        for name in RELATED:
            setattr(nf, name, others)  # independent switches
        def excluded(op, z, pp, **kw):
            """The call keeps the route it has with the switch off, and that is not the new family."""
            got = nf._route(op, z, pp, **kw)
            nf.wide_context_sample_training = False
            try:
                assert got == nf._route(op, z, pp, **kw) and got.family != FAM, (op, got)
            finally:
                nf.wide_context_sample_training = True
            return got.family

        assert nf._route("forward", om, p) == (FAM, False, False)
        assert nf._route("forward", om, p, f32_draw=True) == (FAM, False, False)  # log_q: the caller's
        assert nf._route("forward", om[:, :1], p).family == FAM
        assert nf._route("forward", torch.zeros(3, 31, 5), p).family == FAM
        excluded("forward", torch.zeros(3, 32, 5), p)  # N = 32
        excluded("forward", om[:1], p[:1])  # one parameter row
        assert excluded("forward", om[:1], p) == "bijectors"  # M_z != M
        assert excluded("forward", om, p, freeze_bn=False) == "bijectors"  # fresh statistics
        assert excluded("forward", om, p.detach()) == ("context_rows_wide" if others else "bijectors")  # nothing to train
        with torch.no_grad():
            assert excluded("forward", om, p) == ("context_rows_wide" if others else "bijectors")
        assert excluded("forward", om, p.double()) == "bijectors"
        assert excluded("forward", om.double(), p) == "bijectors"
        assert excluded("forward", om[0], p) == "bijectors"  # 2-d
        assert excluded("log_prob", om, p) == ("train_context_wide" if others else "bijectors")  # sampling only
        assert excluded("inverse", om, p) == "bijectors"
        nf.fusion = _lib.FUSE_LAYER
        assert excluded("forward", om, p) == "bijectors"
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("forward", om, p).family == FAM
        nf.fusion = _lib.FUSE_AUTO
    for b in nf._bn_layers():  # statistics in the graph: only the composition differentiates through them
        b._last_mean = torch.zeros(5, requires_grad=True)
        break
    assert nf._route("forward", om, p).family == "bijectors"
    ar = tnf.NormFlow(5, True, "AR", 1, 2, 20, device="cpu")
    ar.wide_context_sample_training = True
    assert ar._route("forward", om, torch.zeros(3, ar.D_params, requires_grad=True)).family == "bijectors"
    # the unit ranges: 16 stays with train_context_sample, 17 and 64 take the new family
    for U, both, alone in ((15, "train_context_sample", "bijectors"), (16, "train_context_sample", "bijectors"),
                           (17, FAM, FAM), (64, FAM, FAM)):
        f = tnf.NormFlow(5, True, "coupling", 2, 2, U, device="cpu")
        pu = torch.zeros(3, f.D_params, requires_grad=True)
        f.wide_context_sample_training = True
        assert f._route("forward", om, pu).family == alone, U
        f.context_sample_training = True
        assert f._route("forward", om, pu).family == both, U
        f.wide_context_sample_training = False
        assert f._route("forward", om, pu).family == ("train_context_sample" if U <= 16 else "bijectors"), U
    sup = tnf.NormFlow(5, True, "coupling", 2, 2, 20, tnf.ToInterval(5, [-1.0] * 5, [2.0] * 5), device="cpu")
    sup.wide_context_sample_training = True
    ps = torch.zeros(3, sup.D_params, requires_grad=True)
    assert sup._route("forward", om, ps) == (FAM, False, False)  # the support layer: its own op
    # the predicates' depth and LDS refusals
    for L, U, N, fam in ((3, 48, 31, FAM), (4, 20, 8, "bijectors"), (5, 20, 8, "bijectors"), (3, 64, 22, FAM),
                         (3, 64, 23, "bijectors"), (2, 64, 31, FAM), (2, 64, 1, FAM)):
        d64 = tnf.NormFlow(64, True, "coupling", 1, L, U, device="cpu")
        d64.wide_context_sample_training = True
        p64 = torch.zeros(3, d64.D_params, requires_grad=True)
        assert d64._route("forward", torch.zeros(3, N, 64), p64).family == fam, (L, U, N)
    doc = tnf.density_estimator.__doc__
    assert "train_context_    forward (frozen)     wide_context_sample_training (default off)" in doc
    assert "sample_wide" in doc and "ctxwidesample_ops.ctx_" in doc


def test_stats_walk_runs_at_most_once_per_call(monkeypatch):
    calls = []
    real = tnf.NormFlow._stats_in_graph
    monkeypatch.setattr(tnf.NormFlow, "_stats_in_graph", lambda self: (calls.append(1), real(self))[1])
    for kw in (dict(), dict(N=32), dict(rows="one", M=1), dict(stats_graph=True), dict(fusion="LAYER"), dict(D=64, N=1)):
        del calls[:]
        run_row(RT.row(**dict(dict(op="forward", D=5, U=20, S=2, rows="M", M=3, N=31, p_grad=True), **kw)), True)
        assert len(calls) <= 1, (kw, len(calls))


# ---- the algebra of the walk, before any kernel --------------------------------------------------------------------------
def check(tag, gp, go, want, bars):
    from conftest import grad_err

    for name, got, ref, bar in (("params", gp, want[0], bars[0]), ("omega", go, want[1], bars[1])):
        whole, rows = grad_err("ctxwidesample restatement %s %s" % (tag, name), got, ref), R.row_err(got, ref)
        print("ctxwidesample restatement %s %s: whole %.2e per row %.2e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


@pytest.mark.parametrize("group", list(R.groups()))
def test_restatement_against_float64_autograd(oracle, group):
    """float32 gradients from a float32 z, every layer's input rebuilt by the inverse map, explicit deltas, against float64
    autograd through the oracle's composition, over every case of tests/test_gpu_ctx_wide_sample.py; errors whole and per
    context row.  A group's bars are BAR_P and BAR_Z unless the restatement alone exceeds a quarter of one: then 4 x its
    error (`group_bar`), whatever the host.  Measured here (tools/ctxwidesample_grad_restatement.py,
    profiles/r23_ctxwidesample_grad_errors.json), parameters / omega: widths and samples 4.6e-7 / 3.2e-7; S = 1, L = 1
    3.0e-7 / 2.2e-7; S = 1, L = 3 2.7e-7 / 2.1e-7; S = 9, L = 3 8.1e-7 / 5.1e-7; teams and slices 2.9e-7 / 2.7e-7;
    S = 9, L = 1 2.5e-6 / 6.0e-6 at (64, 9, 1, 64) -- the float32 rebuild through 18 one-hidden-layer couplings at
    D = 64, the one computed bar on that host (omega: 2.4e-5)."""
    bars = R.bars(oracle, group)
    for c in R.groups()[group]:
        e = R.restatement_errors(oracle, c)
        print("ctxwidesample restatement %s %s: params %.2e (bar %.1e) omega %.2e (bar %.1e)"
              % (group, R.case_id(c), e["params"], bars[0], e["omega"], bars[1]))
        assert e["params"] <= bars[0] and e["omega"] <= bars[1], (c, e, bars)
    assert BAR_P <= bars[0] < 1e-4 and BAR_Z <= bars[1] < 1e-4, bars  # a computed bar stays a bar: float32 noise, not a bug
    # the walk ends at the draw
    D, S, L, U, M, N = c = R.groups()[group][-1]
    params, mean, alpha, omega = CF.inputs(oracle, *c)
    z = R.forward32(oracle, omega, params, mean, alpha, (D, S, L, U))
    assert z.dtype == torch.float32
    gp, go, om = R.sample_bwd(z, params, mean, alpha, *R.upstream(M, N, D), D, S, L, U)
    assert gp.shape == params.shape and go.shape == omega.shape and gp.dtype == go.dtype == torch.float32
    torch.testing.assert_close(om, omega, rtol=1e-4, atol=1e-4)  # (domain_helpers.INV_TOL)


@pytest.mark.parametrize("D,S,L,U,M,N", R.ONE_COTANGENT, ids=lambda v: str(v))
def test_restatement_one_upstream_gradient_at_a_time(oracle, D, S, L, U, M, N):
    params, mean, alpha, omega = CF.inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    shape = (D, S, L, U)
    z = R.forward32(oracle, omega, params, mean, alpha, shape)
    for tag, a, b in (("g_z only", g_z, None), ("g_sld only", None, g_sld)):
        gp, go, _ = R.sample_bwd(z, params, mean, alpha, a, b, *shape)
        check("%s D=%d N=%d" % (tag, D, N), gp, go, R.reference(oracle, float64, omega, params, mean, alpha, a, b, shape),
              (BAR_P, BAR_Z))
    gp, go, _ = R.sample_bwd(z, params, mean, alpha, torch.zeros_like(g_z), torch.zeros_like(g_sld), *shape)
    assert not gp.any() and not go.any()  # zero upstream gradient: exactly zero everywhere
