"""The whole-flow wide kernel (include/tnf_wideflow.h, csrc/flow_wide.hip, NormFlow's family `wide_flow`), without a GPU:
header, exports and binding table in step; the support predicate over a grid against its restated definition; every
refusal that precedes a launch; the restated formulation against the oracle in float64, with planted defects that must
fail; every case of the GPU sweep's grid finds its inputs; and the routing of NormFlow with the switch on and off."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import test_route_table as RT
import wideflow_restatement as W
from domain_helpers import float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, wideflow_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
HEADER = os.path.join(ROOT, "include", "tnf_wideflow.h")
OTHER_TABLES = ("SIGNATURES", "MOG_SIGNATURES", "ABC_SIGNATURES", "HEBB_SIGNATURES", "EFN_SIGNATURES", "PADTRAIN_SIGNATURES",
                "PADBATCH_SIGNATURES", "CTXFLOW_SIGNATURES", "CTXTRAIN_SIGNATURES", "SAMPLETRAIN_SIGNATURES",
                "ARSAMPLE_SIGNATURES", "ARBATCH_SIGNATURES", "CTXSAMPLE_SIGNATURES")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.WIDEFLOW_SIGNATURES) and len(protos) == 4
    tables = [n for n in dir(_lib) if n.endswith("SIGNATURES") and n != "WIDEFLOW_SIGNATURES"]
    assert set(OTHER_TABLES) <= set(tables)
    for n in tables:
        assert not set(_lib.WIDEFLOW_SIGNATURES) & set(getattr(_lib, n)), n
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.WIDEFLOW_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.WIDEFLOW_SIGNATURES["tnf_wide_flow_launch_count"][0] is ctypes.c_int64
    header = open(HEADER).read()
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_wideflow.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    for i, n in enumerate(("LOG_PROB", "FORWARD")):
        assert "TNF_WIDEFLOW_COUNT_%s = %d" % (n, i) in header
    assert "TNF_WIDEFLOW_COUNTERS = 2" in header
    assert (wideflow_ops.COUNT_LOG_PROB, wideflow_ops.COUNT_FORWARD) == (0, 1)
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(2):
        assert lib.tnf_wide_flow_launch_count(which) >= 0
    assert lib.tnf_wide_flow_launch_count(2) == -1 and b"tnf_wide_flow_launch_count" in lib.tnf_last_error()
    assert lib.tnf_wide_flow_launch_count(-1) == -1


def test_predicate_is_its_definition_over_the_grid():
    """Every bound bracketed: D, U and L one below, at and one above; S from 0 to one past the largest that fits, for each
    (HT, UT, L)."""
    ones = 0
    for D in (1, 2, 31, 32, 33, 34, 64, 65):
        for U in (16, 17, 32, 33, 48, 49, 64, 65):
            for L in (0, 1, 2, 3, 4, 5, 6):
                top = W.largest_S(D, max(L, 1), U)
                for S in range(0, top + 2):
                    want = W.wide_flow_supported(D, S, L, U)
                    assert lib.tnf_wide_flow_supported(D, S, L, U) == int(want), (D, S, L, U)
                    assert wideflow_ops.wide_flow_supported(D, S, L, U) == want
                    ones += want
                if 2 <= D <= 64 and 17 <= U <= 64 and 1 <= L <= 5:  # the budget is the bound that binds
                    assert [W.wide_flow_supported(D, S, L, U) for S in (top, top + 1)] == [top >= 1, False]
    assert ones > 200
    # the header's table at L = 2
    assert [W.largest_S(D, 2, U) for D, U in ((32, 32), (33, 32), (64, 32), (32, 48), (32, 64), (64, 64))] == [4, 2, 2, 2, 1, 1]
    assert W.lds_bytes(32, 4, 2, 32) == 138240 and W.lds_bytes(64, 1, 2, 64) == 134656
    assert [lib.tnf_wide_flow_supported(*s) for s in W.sweep_shapes(refused=True)] == [0, 0]  # UT = 4, L = 3: no S fits
    assert lib.tnf_wide_flow_supported(4, 1 << 30, 2, 20) == 0 and lib.tnf_wide_flow_supported(4, -1, 2, 20) == 0
    assert lib.tnf_wide_flow_supported(4, 1, 2, 15) == 0 and lib.tnf_wide_flow_supported(4, 1, 2, 16) == 0  # not claimed


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    counts = wideflow_ops.launch_counts()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 20)
    assert P5 == W.flow_params(5, 2, 2, 20)

    def log_prob(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], lp=p[4], z0=p[5], sld=p[6], Mz=3, Mp=3, N=8, D=5, S=2, L=2, U=20,
                 pstride=P5)
        a.update(kw)
        return lib.tnf_wide_flow_log_prob_f32(a["z"], a["params"], a["mean"], a["alpha"], a["lp"], a["z0"], a["sld"],
                                              a["Mz"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    def forward(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], z0=p[5], sld=p[6], Mz=3, Mp=3, N=8, D=5, S=2, L=2, U=20, pstride=P5)
        a.update(kw)
        return lib.tnf_wide_flow_forward_f32(a["z"], a["params"], a["mean"], a["alpha"], a["z0"], a["sld"], a["Mz"], a["Mp"],
                                             a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    unsupported = (dict(D=1), dict(D=65), dict(D=0), dict(L=6), dict(L=0), dict(U=16), dict(U=65), dict(U=0), dict(S=0),
                   dict(S=W.largest_S(5, 2, 20) + 1), dict(U=64, L=3, S=1))
    for call, tag in ((log_prob, b"tnf_wide_flow_log_prob_f32"), (forward, b"tnf_wide_flow_forward_f32")):
        for name in ("z", "params", "mean", "alpha"):
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in (dict(Mz=0, Mp=0), dict(Mz=-3), dict(Mp=0), dict(N=-1), dict(Mz=2), dict(Mp=2), dict(Mz=4, Mp=3)):
            refused(call(**kw), INV, tag + b": M_z=")
        for kw in unsupported:
            refused(call(**kw), UNSUP, tag + b": no whole-flow wide kernel for D=")
        refused(call(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
        assert call(N=0) == 0  # nothing to do: OK, no launch
        assert call(Mp=1, N=0) == 0  # one shared parameter row
        refused(call(N=0, pstride=P5 - 1), INV, tag + b": params row has")  # ... after the other checks
    refused(log_prob(lp=None, z0=None, sld=None), INV, b"tnf_wide_flow_log_prob_f32: no output requested")
    refused(forward(z0=None, sld=None), INV, b"tnf_wide_flow_forward_f32: no output requested")
    refused(forward(Mz=1, Mp=3), INV, b"tnf_wide_flow_forward_f32: M_z=1 M_p=3")  # sampling: one block of draws per row
    refused(log_prob(z0=p[0]), INV, b"z0 must not alias z")
    refused(forward(z0=p[0]), INV, b"z_out must not alias omega")
    assert log_prob(Mz=1, N=0) == 0 and log_prob(lp=None, sld=None, N=0) == 0 and forward(sld=None, N=0) == 0
    assert wideflow_ops.launch_counts() == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- the restatement ---------------------------------------------------------------------------------------------------
RESTATED = [(2, 1, 2, 20), (3, 2, 2, 17), (4, 1, 2, 20), (5, 2, 3, 33), (8, 1, 1, 64), (31, 1, 2, 48), (33, 2, 2, 20), (64, 1, 2, 64)]


@pytest.fixture(scope="module")
def cases(oracle):
    return {s: W.Case(oracle, *s) for s in RESTATED}


@pytest.mark.parametrize("shape", RESTATED, ids=W.case_id)
def test_restatement_is_the_oracle_in_float64(cases, shape):
    """Even and odd D, D = 2 and 3, both directions, M_p = 1 and 3 (and one block of z for three rows): 1e-12."""
    c = cases[shape]
    for Mz, Mp in W.LAYOUTS:
        z, p = c.inputs(Mz, Mp)
        want, sc = c.want(Mz, Mp, W.N_FULL), c.scale()
        with float64(), torch.no_grad():
            lp, z0, sld = W.wide_flow_log_prob(z.double(), p.double(), *shape, c.stat)
            got = dict(lp=lp, z0=z0, sld=sld)
            if Mz >= Mp:
                zf, sldf, pad = W.wide_flow_forward(z.double(), p.double(), *shape, c.stat)
                got.update(zf=zf, sldf=sldf)
                assert pad == 0.0  # the padding stays exactly 0 through every layer
        for k, v in got.items():
            assert v.dtype == torch.float64 and v.shape == want[k].shape
            assert W.err(v, want[k], sc[k]) <= 1e-12, (k, Mz, Mp)


@pytest.mark.parametrize("defect", ["pad_weight", "pad_fold"])
@pytest.mark.parametrize("shape", [(3, 2, 2, 17), (5, 2, 3, 33), (33, 2, 2, 20)], ids=W.case_id)
def test_planted_defects_fail(cases, shape, defect):
    """A non-zero operand in a padded slot of the image, or a padded slot of the fold that is not (1, 0), breaks the
    float64 agreement by many orders of magnitude: the check above can fail."""
    c = cases[shape]
    z, p = c.inputs(3, 3)
    with float64(), torch.no_grad():
        lp = W.wide_flow_log_prob(z.double(), p.double(), *shape, c.stat, defect=defect)[0]
        good = W.wide_flow_log_prob(z.double(), p.double(), *shape, c.stat)[0]
    want = c.want(3, 3, W.N_FULL)["lp"]
    assert W.err(good, want) <= 1e-12 < 1e-7 < W.err(lp, want)


def test_every_case_of_the_sweep_finds_its_inputs(oracle):
    """The grid covers what it must, and every case has a seed whose float64 references stay below 1e3 (a RuntimeError
    otherwise: no case is skipped)."""
    shapes = W.sweep_shapes()
    assert {s[0] for s in shapes} == {2, 3, 5, 8, 31, 32, 33, 63, 64} and {s[3] for s in shapes} == {17, 20, 32, 33, 48, 64}
    cells = {W.tiles(D, U) + (L,) for D, S, L, U in shapes}
    assert cells == {(HT, UT, L) for HT in (1, 2) for UT in (2, 3, 4) for L in (1, 2, 3) if (UT, L) != (4, 3)} | {(1, 2, 5)}
    assert {1, 2} <= {s[1] for s in shapes} and sum(s[1] == W.largest_S(s[0], s[2], s[3]) > 2 for s in shapes) >= 2
    assert all(W.wide_flow_supported(*s) for s in shapes)
    for s in shapes + list(W.WALK_SHAPES.values()) + [W.CDE_SHAPE]:
        c = W.Case(oracle, *s)
        assert 0 <= c.seed < W.SEEDS and all(0.0 < v < 1e-3 for v in c.noise().values()), s
    for HT, s in W.WALK_SHAPES.items():
        assert W.tiles(s[0], s[3])[0] == HT
        assert W.grid_x(W.WALK_N, 1) == 17 and W.grid_x(W.WALK_N, W.WALK_M) == 1  # waves without a tile; waves with 17


# ---- routing -----------------------------------------------------------------------------------------------------------------
LP, FWD = "wide_flow_log_prob_raw", "wide_flow_forward_raw"
TODAY = ("affine", "coupling", "flow_log_prob_raw", "flow_forward_raw")  # the composition, or the wide per-layer chain


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.wide_flow` = switch and the two new entries recorded."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tnf.NormFlow, "wide_flow", switch)
        trace = []
        for name in (LP, FWD):
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(wideflow_ops, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_wide_flow(r):
    """The conditions of the new row of the routing docstring, from the grid row alone -> LP, FWD or None."""
    forward = r["op"] == "forward"
    if not (r["arch"] == "coupling" and (r["freeze_bn"] or not forward) and r["fusion"] != "LAYER"
            and (forward or r["zdim"] == 3) and not (r["sup"] and r["op"] == "inverse")
            and W.wide_flow_supported(r["D"], r["S"], RT.L, r["U"])):
        return None
    if not forward and r["zdtype"] != "float32":
        return None
    if r["rows"] == "M" and r["M"] > 1 and (r["N"] < 32 or (forward and r["D"] in (8, 16, 24))):
        return None  # (the second: the one measured exclusion)
    plain = r["no_grad"] or not (r["p_grad"] or (r["z_grad"] and not forward))
    if not plain or (r["stats_graph"] and not r["no_grad"]):
        return None
    return FWD if forward else LP


def test_every_row_of_the_grid_on_and_off():
    """Switch off: every route of the recorded table is unchanged.  Switch on: a row changes exactly when the conditions
    of the new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), {LP: 0, FWD: 0}
    for i, r in enumerate(RT.GRID):
        old = table[RT.row_id(r)]
        want = takes_wide_flow(r)
        if want is None and (r["U"] <= 16 and i % 7):  # every row above 16 units, every seventh of the others
            continue
        assert run_row(r, False) == old, RT.row_id(r)
        on = run_row(r, True)
        if want is not None and not old[-1].startswith("raises"):
            assert old[-1].split("(")[0] in TODAY, RT.row_id(r)
            assert on == old[:-1] + [want], RT.row_id(r)
            changed[want] += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed[LP] >= 10 and changed[FWD] >= 5, changed  # not vacuous


def _flow(D, S, L, U, arch="coupling", **kw):
    nf = tnf.NormFlow(D, True, arch, S, L, U, device="cpu", **kw)
    return nf, torch.zeros(3, nf.D_params)


def test_switch_over_the_predicate_grid():
    """Over the shapes that bracket the predicate: off, `_route` answers as it does with the family removed; on, it answers
    `wide_flow` exactly where the definition says."""
    for D in (2, 5, 8, 32, 33, 64, 65):
        for U in (15, 16, 17, 64, 65):
            for L in (1, 5, 6):
                top = max(W.largest_S(min(D, 64), min(L, 5), min(max(U, 17), 64)), 1)
                for S in (1, top, top + 1):
                    nf, p = _flow(D, S, L, U)
                    for op, z in (("log_prob", torch.zeros(1, 40, D)), ("inverse", torch.zeros(3, 40, D)),
                                  ("forward", torch.zeros(3, 40, D))):
                        pp = p if z.shape[0] == 3 else p[:1]
                        with torch.no_grad():
                            with pytest.MonkeyPatch.context() as mp:
                                mp.setattr(tnf.NormFlow, "_wide_flow_ok", lambda *a, **k: False)
                                before = nf._route(op, z, pp)
                            assert nf._route(op, z, pp) == before and before.family != "wide_flow"
                            nf.wide_flow = True
                            on = nf._route(op, z, pp)
                            nf.wide_flow = False
                        slower = op == "forward" and D == 8  # several rows at D % 8 == 0 < 32: measured, DESIGN.md 24
                        if W.wide_flow_supported(D, S, L, U) and not slower:
                            assert on == ("wide_flow", False, False), (D, S, L, U, op)
                        else:
                            assert on == before, (D, S, L, U, op)


def test_exclusions_take_todays_route():
    nf, p = _flow(8, 1, 2, 20)
    z = torch.zeros(3, 40, 8)
    with torch.no_grad():
        off = {op: nf._route(op, z, p) for op in ("log_prob", "inverse", "forward")}
        assert all(r.family == "fused" for r in off.values())  # D % 8 == 0: the wide per-layer chain
        nf.wide_flow = True
        for op in off:
            # sampling with several rows at D % 8 == 0 below 32 was measured slower than the wide chain: left to it
            assert nf._route(op, z, p) == (off[op] if op == "forward" else ("wide_flow", False, False))
            assert nf._route(op, z, p[:1]) == ("wide_flow", False, False)  # one shared row
        assert nf._route("forward", z, p[:1], f32_draw=True) == ("wide_flow", False, False)  # the caller forms log_q
        d32, p32 = _flow(32, 1, 2, 20)
        d32.wide_flow = True
        assert d32._route("forward", torch.zeros(3, 40, 32), p32).family == "wide_flow"  # ... from D = 32 on it is not
        assert nf._route("log_prob", z[:1], p).family == "wide_flow"  # one block of z
        assert nf._route("forward", z, p, freeze_bn=False) == nf.__class__._route(nf, "forward", z, p, False)
        assert nf._route("forward", z, p, freeze_bn=False).family != "wide_flow"  # fresh statistics
        assert nf._route("log_prob", z[:, :31], p) == off["log_prob"]._replace(family="bijectors")  # rows with N < 32
        assert nf._route("log_prob", z[:, :31], p[:1]).family == "wide_flow"  # ... but any N with one row
        assert nf._route("log_prob", z[0], p[:1]).family != "wide_flow"  # 2-d z
        assert nf._route("log_prob", z.double(), p).family == "bijectors"
        nf.fusion = _lib.FUSE_LAYER
        assert nf._route("log_prob", z, p) == off["log_prob"]  # FUSE_LAYER keeps the per-layer chain
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("log_prob", z, p).family == "wide_flow"
        nf.fusion = _lib.FUSE_AUTO
    pg = p.clone().requires_grad_()
    assert nf._route("log_prob", z, pg).family not in ("wide_flow", "fused")  # autograd keeps today's routes
    assert nf._route("forward", z, pg).family != "wide_flow"
    assert nf._route("log_prob", z.clone().requires_grad_(), p).family != "wide_flow"
    assert nf._route("log_prob", z, p).family == "wide_flow"  # grad mode on, nothing requires grad: plain
    with torch.no_grad():
        for U in (15, 16):
            narrow, pn = _flow(8, 1, 2, U)
            narrow.wide_flow = True
            assert narrow._route("log_prob", z, pn).family == "padded"  # U <= 16: the split-f16 kernels keep them
        ar, pa = _flow(8, 1, 2, 20, arch="AR")
        ar.wide_flow = True
        assert ar._route("log_prob", z, pa).family == "ar_fused"
        sup, ps = _flow(8, 1, 2, 20, support_layer=tnf.ToInterval(8, [-1.0] * 8, [2.0] * 8))
        sup.wide_flow = True
        assert sup._route("log_prob", z, ps) == ("wide_flow", False, False)  # the support layer: its own kernel
        assert sup._route("forward", z, ps[:1]) == ("wide_flow", False, False)
        assert sup._route("inverse", z, ps).family == "bijectors"
        odd, po = _flow(5, 1, 2, 20)
        assert odd._route("log_prob", torch.zeros(3, 40, 5), po).family == "bijectors"
        odd.wide_flow = True
        assert odd._route("log_prob", torch.zeros(3, 40, 5), po).family == "wide_flow"


def test_switch_defaults_to_off():
    assert tnf.NormFlow.wide_flow is False
    nf, p = _flow(4, 1, 2, 20)
    assert "wide_flow" not in vars(nf)
    with torch.no_grad():
        assert nf._route("log_prob", torch.zeros(1, 33, 4), p[:1]).family == "bijectors"
        nf.wide_flow = True
        assert nf._route("log_prob", torch.zeros(1, 33, 4), p[:1]).family == "wide_flow"
