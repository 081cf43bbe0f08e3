"""The streamed whole-flow wide kernel (include/tnf_widestream.h, csrc/flow_wide_stream.hip, NormFlow's family
`wide_flow_streamed`), without a GPU: header, exports and binding table in step; the support predicate, the LDS size and
the tile rule over a grid against their restated definitions; every refusal that precedes a launch; the routing of
NormFlow with the switch on and off; and the restated formulation of tests/wideflow_restatement.py against the oracle in
float64 at the GPU sweep's shapes, whose stage counts lie beyond what test_wideflow_host.py verifies it at."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
import test_route_table as RT
import wideflow_restatement as W
import widestream_restatement as R
from domain_helpers import float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, wideflow_ops, widestream_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
HEADER = os.path.join(ROOT, "include", "tnf_widestream.h")
TABLE = "WIDESTREAM_ENTRIES"
NAMES = ("tnf_wide_flow_stream_supported", "tnf_wide_flow_stream_lds_bytes", "tnf_wide_flow_stream_tiles",
         "tnf_wide_flow_stream_set_tiles", "tnf_wide_flow_stream_launch_count", "tnf_wide_flow_stream_log_prob_f32",
         "tnf_wide_flow_stream_forward_f32")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    table = getattr(_lib, TABLE)
    assert sorted(protos) == sorted(table) == sorted(NAMES)
    # the `*_SIGNATURES` tables are a closed set of fifteen (test_ctx_wide_sample_host.py), so this one is named as
    # CTXWIDESAMPLE_ENTRIES is; the new names appear in no other table
    others = [n for n in dir(_lib) if (n.endswith("SIGNATURES") or n.endswith("_ENTRIES")) and n != TABLE]
    assert len(others) == 16 and "CTXWIDESAMPLE_ENTRIES" in others
    for n in others:
        assert not set(table) & set(getattr(_lib, n)), n
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = table[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    for name in ("tnf_wide_flow_stream_launch_count", "tnf_wide_flow_stream_lds_bytes"):
        assert table[name][0] is ctypes.c_int64
    header = open(HEADER).read()
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_widestream.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    for i, n in enumerate(("LOG_PROB", "FORWARD")):
        assert "TNF_WIDESTREAM_COUNT_%s = %d" % (n, i) in header
    assert "TNF_WIDESTREAM_COUNTERS = 2" in header
    assert (widestream_ops.COUNT_LOG_PROB, widestream_ops.COUNT_FORWARD) == (0, 1)
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(2):
        assert lib.tnf_wide_flow_stream_launch_count(which) >= 0
    assert lib.tnf_wide_flow_stream_launch_count(2) == -1 and b"tnf_wide_flow_stream_launch_count" in lib.tnf_last_error()
    assert lib.tnf_wide_flow_stream_launch_count(-1) == -1


GRID_D, GRID_U = (1, 2, 32, 33, 64, 65), (16, 17, 32, 33, 48, 49, 64, 65)
GRID_L, GRID_S = tuple(range(0, 7)), (0, 1, 5, 1024, 1025, 1 << 30, -1)


def test_predicate_and_lds_are_their_definitions_over_the_grid():
    ones = resident = 0
    for D in GRID_D:
        for U in GRID_U:
            for L in GRID_L:
                assert lib.tnf_wide_flow_stream_lds_bytes(D, L, U) == R.lds_bytes(D, L, U) == widestream_ops.lds_bytes(D, L, U)
                assert (R.lds_bytes(D, L, U) > 0) == R.in_domain(D, L, U) and R.lds_bytes(D, L, U) <= W.LDS_BUDGET
                for S in GRID_S:
                    want = R.supported(D, S, L, U)
                    assert lib.tnf_wide_flow_stream_supported(D, S, L, U) == int(want), (D, S, L, U)
                    assert widestream_ops.wide_flow_stream_supported(D, S, L, U) == want
                    ones += want
                    # the resident kernel keeps its values, and what it covers is covered here too
                    assert lib.tnf_wide_flow_supported(D, S, L, U) == int(W.wide_flow_supported(D, S, L, U))
                    if W.wide_flow_supported(D, S, L, U):
                        assert want
                        resident += 1
    assert ones > 300 and resident > 50
    # the pinned values
    assert (W.layer_floats(64, 2, 64) * 4, R.slots(64, 2, 64), lib.tnf_wide_flow_stream_lds_bytes(64, 2, 64)) == (67328, 2, 134656)
    assert (R.slots(8, 5, 64), lib.tnf_wide_flow_stream_lds_bytes(8, 5, 64)) == (1, 150400)
    assert W.layer_floats(64, 5, 64) * 4 == 167168 and lib.tnf_wide_flow_stream_lds_bytes(64, 5, 64) == 0
    assert [lib.tnf_wide_flow_stream_supported(64, S, 5, 64) for S in (1, 2)] == [0, 0]
    assert [lib.tnf_wide_flow_stream_supported(64, S, 2, 64) for S in (1, 4, 1024, 1025)] == [1, 1, 1, 0]
    assert lib.tnf_wide_flow_stream_supported(8, 7, 5, 64) == 1
    # the sweep: every shape is streamed-only, with the slot counts the GPU tests rely on
    assert len(R.SWEEP) == 16 and all(R.supported(*s) and not W.wide_flow_supported(*s) for s in R.SWEEP)
    assert [s for s in R.SWEEP if R.slots(s[0], s[2], s[3]) == 1] == R.ONE_SLOT
    assert all(sum(s[2] == L for s in R.SWEEP) >= 2 for L in (1, 2, 3, 4, 5))
    assert all(R.supported(*s) and W.wide_flow_supported(*s) for s in R.BOTH)
    assert all(R.supported(*s) and not W.wide_flow_supported(*s) for s in R.WALK_SHAPES + [R.NF_SHAPE, R.CDE_SHAPE])


def test_tile_rule_and_override():
    for D, L, U in ((5, 2, 20), (33, 2, 20), (64, 2, 64), (64, 4, 64), (64, 3, 64), (8, 5, 64), (32, 2, 32)):
        for M in (1, 2, 129, 256, 2000):
            for N in (1, 100, 128, 129, 273, 1041, 1 << 12, 1 << 15, 1 << 17, 1 << 20):
                want = R.tiles(D, L, U, M, N)
                assert lib.tnf_wide_flow_stream_tiles(D, 3, L, U, M, N) == want, (D, L, U, M, N)
                assert want in R.SHIPPED_TILES and want <= R.max_tiles(D, L, U)
    assert R.tiles(5, 2, 20, 2000, 100) == 1  # rows of about 100 samples: seven tiles
    assert R.tiles(5, 2, 20, 1, 1 << 20) == 4 and R.tiles(64, 2, 64, 1, 1 << 20) == 2 and R.tiles(64, 4, 64, 1, 1 << 20) == 1
    assert R.tiles(5, 2, 20, 1, 1 << 15) == 1  # 2,048 tiles: 256 groups only at T = 1
    assert lib.tnf_wide_flow_stream_tiles(5, 0, 2, 20, 1, 100) == -1 and lib.tnf_wide_flow_stream_tiles(5, 1, 2, 16, 1, 100) == -1
    assert lib.tnf_wide_flow_stream_tiles(5, 1, 2, 20, 0, 100) == -1 and lib.tnf_wide_flow_stream_tiles(5, 1, 2, 20, 1, -1) == -1
    assert widestream_ops.SHIPPED_TILES == R.SHIPPED_TILES
    assert lib.tnf_wide_flow_stream_set_tiles(0) == 0  # the default: the rule
    try:
        for T in R.SHIPPED_TILES:
            prev = widestream_ops.set_tiles(T)
            assert widestream_ops.set_tiles(T) == T and prev in (0,) + R.SHIPPED_TILES
            assert lib.tnf_wide_flow_stream_tiles(5, 1, 2, 20, 2000, 100) == 1  # the rule's answer, not the override
        for bad in (3, 8, -1, 5):
            assert lib.tnf_wide_flow_stream_set_tiles(bad) == INV and b"tnf_wide_flow_stream_set_tiles" in lib.tnf_last_error()
            assert lib.tnf_wide_flow_stream_set_tiles(4) == 4  # a refused value changed nothing
    finally:
        lib.tnf_wide_flow_stream_set_tiles(0)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    counts, wide = widestream_ops.launch_counts(), wideflow_ops.launch_counts()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 9, 2, 20)
    assert P5 == W.flow_params(5, 9, 2, 20)

    def log_prob(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], lp=p[4], z0=p[5], sld=p[6], Mz=3, Mp=3, N=8, D=5, S=9, L=2, U=20,
                 pstride=P5)
        a.update(kw)
        return lib.tnf_wide_flow_stream_log_prob_f32(a["z"], a["params"], a["mean"], a["alpha"], a["lp"], a["z0"], a["sld"],
                                                     a["Mz"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    def forward(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], z0=p[5], sld=p[6], Mz=3, Mp=3, N=8, D=5, S=9, L=2, U=20, pstride=P5)
        a.update(kw)
        return lib.tnf_wide_flow_stream_forward_f32(a["z"], a["params"], a["mean"], a["alpha"], a["z0"], a["sld"], a["Mz"],
                                                    a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    unsupported = (dict(D=1), dict(D=65), dict(D=0), dict(L=6), dict(L=0), dict(U=16), dict(U=65), dict(U=0), dict(S=0),
                   dict(S=-1), dict(S=1025), dict(S=1 << 30), dict(D=64, U=64, L=5, S=1), dict(D=33, U=49, L=5, S=1))
    for call, tag in ((log_prob, b"tnf_wide_flow_stream_log_prob_f32"), (forward, b"tnf_wide_flow_stream_forward_f32")):
        for name in ("z", "params", "mean", "alpha"):
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in (dict(Mz=0, Mp=0), dict(Mz=-3), dict(Mp=0), dict(N=-1), dict(Mz=2), dict(Mp=2), dict(Mz=4, Mp=3)):
            refused(call(**kw), INV, tag + b": M_z=")
        refused(call(Mz=32768 * 65535 + 1, Mp=1), INV, tag + b": M=")
        for kw in unsupported:
            refused(call(**kw), UNSUP, tag + b": no streamed whole-flow wide kernel for D=")
        refused(call(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
        assert call(N=0) == 0  # nothing to do: OK, no launch
        assert call(Mp=1, N=0) == 0  # one shared parameter row
        refused(call(N=0, pstride=P5 - 1), INV, tag + b": params row has")  # ... after the other checks
    refused(log_prob(lp=None, z0=None, sld=None), INV, b"tnf_wide_flow_stream_log_prob_f32: no output requested")
    refused(forward(z0=None, sld=None), INV, b"tnf_wide_flow_stream_forward_f32: no output requested")
    refused(forward(Mz=1, Mp=3), INV, b"tnf_wide_flow_stream_forward_f32: M_z=1 M_p=3")  # sampling: one block of draws per row
    refused(log_prob(z0=p[0]), INV, b"z0 must not alias z")
    refused(forward(z0=p[0]), INV, b"z_out must not alias omega")
    # the order: NULL input, no output, the M's, the shape, pstride, aliasing
    refused(log_prob(z=None, lp=None, z0=None, sld=None, Mz=0), INV, b"NULL pointer")
    refused(log_prob(lp=None, z0=None, sld=None, Mz=0), INV, b"no output requested")
    refused(log_prob(Mz=0, D=1), INV, b": M_z=")
    refused(log_prob(D=1, pstride=0), UNSUP, b"no streamed whole-flow wide kernel")
    refused(log_prob(pstride=P5 - 1, z0=p[0]), INV, b"params row has")
    assert log_prob(Mz=1, N=0) == 0 and log_prob(lp=None, sld=None, N=0) == 0 and forward(sld=None, N=0) == 0
    assert widestream_ops.launch_counts() == counts and wideflow_ops.launch_counts() == wide  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- the restatement beyond the resident kernel's stage counts ---------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(oracle):
    return {}


@pytest.mark.parametrize("shape", R.SWEEP, ids=W.case_id)
def test_restatement_is_the_oracle_in_float64(oracle, cases, shape):
    """The reference of the GPU sweep's bars at its own shapes -- S up to 9 -- both directions, every layout: 1e-12."""
    c = cases.setdefault(shape, W.Case(oracle, *shape))
    assert 0 <= c.seed < W.SEEDS and all(0.0 < v < 1e-3 for v in c.noise().values()), shape
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


# ---- routing -----------------------------------------------------------------------------------------------------------------
LP, FWD = "wide_flow_stream_log_prob_raw", "wide_flow_stream_forward_raw"
RES_LP, RES_FWD = "wide_flow_log_prob_raw", "wide_flow_forward_raw"
TODAY = ("affine", "coupling", "flow_log_prob_raw", "flow_forward_raw")  # the composition, or the wide per-layer chain


def run_row(r, streamed, resident=False):
    """test_route_table.run_row with the two switches set and the entries of both families recorded."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tnf.NormFlow, "wide_flow_streamed", streamed)
        mp.setattr(tnf.NormFlow, "wide_flow", resident)
        trace = []
        for mod, names in ((widestream_ops, (LP, FWD)), (wideflow_ops, (RES_LP, RES_FWD))):
            for name in names:
                def recorder(*args, _name=name, **kwargs):
                    trace.append(_name)
                    raise RT._Reached()

                mp.setattr(mod, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def inference_row(r):
    """The conditions the two wide families share (the docstring's row of `wide_flow`), but the shape, from the grid row."""
    forward = r["op"] == "forward"
    if not (r["arch"] == "coupling" and (r["freeze_bn"] or not forward) and r["fusion"] != "LAYER"
            and (forward or r["zdim"] == 3) and not (r["sup"] and r["op"] == "inverse")):
        return False
    if not forward and r["zdtype"] != "float32":
        return False
    if r["rows"] == "M" and r["M"] > 1 and r["N"] < 32:
        return False
    plain = r["no_grad"] or not (r["p_grad"] or (r["z_grad"] and not forward))
    return plain and not (r["stats_graph"] and not r["no_grad"])


def takes_streamed(r):
    """The new row of the routing docstring -> LP, FWD or None."""
    shape = (r["D"], r["S"], RT.L, r["U"])
    if not (inference_row(r) and not W.wide_flow_supported(*shape) and R.supported(*shape)):
        return None
    if r["D"] % 8 == 0 and not (r["M"] == 1 and r["N"] <= 1 << (12 if r["op"] == "forward" else 17)):
        return None  # (the one measured exclusion)
    return FWD if r["op"] == "forward" else LP


def test_every_row_of_the_grid_on_and_off():
    """Switch off: every route of the recorded table is unchanged.  Switch on: a row changes exactly when the conditions of
    the new family hold, and then only in its last entry.  Both switches on: what the resident kernel covers stays with
    it, and the streamed rows are the same."""
    table, changed, resident = RT._table(), {LP: 0, FWD: 0}, 0
    for i, r in enumerate(RT.GRID):
        old = table[RT.row_id(r)]
        want = takes_streamed(r)
        if want is None and (r["U"] <= 16 and i % 7):  # every row above 16 units, every seventh of the others
            continue
        assert run_row(r, False) == old, RT.row_id(r)
        on = run_row(r, True)
        both = run_row(r, True, True)
        if want is not None and not old[-1].startswith("raises"):
            assert old[-1].split("(")[0] in TODAY, RT.row_id(r)
            assert on == both == old[:-1] + [want], RT.row_id(r)
            changed[want] += 1
        else:
            assert on == old, RT.row_id(r)  # the new switch alone: resident shapes keep today's route
            assert both == run_row(r, False, True), RT.row_id(r)
            assert not set(both) & {LP, FWD}
            resident += both[-1] in (RES_LP, RES_FWD)
    assert changed[LP] >= 6 and changed[FWD] >= 3 and resident >= 15, (changed, resident)  # not vacuous


def _flow(D, S, L, U, arch="coupling", **kw):
    nf = tnf.NormFlow(D, True, arch, S, L, U, device="cpu", **kw)
    return nf, torch.zeros(3, nf.D_params)


def test_switch_defaults_to_off():
    assert tnf.NormFlow.wide_flow_streamed is False
    nf, p = _flow(64, 4, 2, 64)
    assert "wide_flow_streamed" not in vars(nf)
    with torch.no_grad():
        z = torch.zeros(1, 33, 64)
        off = nf._route("log_prob", z, p[:1])
        assert off.family == "fused"  # D % 8 == 0: the wide per-layer chain
        nf.wide_flow = True
        assert nf._route("log_prob", z, p[:1]) == off  # the resident kernel cannot hold S = 4 at 64 units
        nf.wide_flow = False
        nf.wide_flow_streamed = True
        assert nf._route("log_prob", z, p[:1]) == ("wide_flow_streamed", False, False)


def test_the_two_families_are_disjoint_and_the_exclusions_hold():
    with torch.no_grad():
        for D, S, L, U in ((5, 1, 2, 20), (5, 5, 2, 20), (33, 2, 2, 20), (33, 3, 2, 20), (64, 1, 2, 64), (64, 2, 2, 64),
                           (64, 1, 3, 64), (64, 1, 5, 64), (8, 1, 2, 20), (8, 5, 2, 20), (8, 1, 2, 16), (8, 5, 2, 65)):
            nf, p = _flow(D, S, L, U)
            z = torch.zeros(1, 40, D)
            res, stream = W.wide_flow_supported(D, S, L, nf.num_units), R.supported(D, S, L, nf.num_units)
            for op in ("log_prob", "inverse", "forward"):
                off = nf._route(op, z, p[:1])
                assert off.family not in ("wide_flow", "wide_flow_streamed")
                nf.wide_flow_streamed = True
                on = nf._route(op, z, p[:1])
                assert on == (("wide_flow_streamed", False, False) if stream and not res else off), (D, S, L, U, op)
                nf.wide_flow = True
                both = nf._route(op, z, p[:1])
                assert both.family == ("wide_flow" if res else "wide_flow_streamed" if stream else off.family)
                nf.wide_flow = nf.wide_flow_streamed = False
        # D % 8 == 0, where today's route is the wide per-layer chain: only one block of z, one parameter row, N <= 2^17
        d8, p8 = _flow(8, 5, 2, 20)
        z8 = torch.zeros(3, 40, 8)
        off8 = {op: d8._route(op, z8, p8) for op in ("log_prob", "inverse", "forward")}
        assert all(r.family == "fused" for r in off8.values())
        d8.wide_flow_streamed = True
        for op in off8:
            assert d8._route(op, z8, p8) == off8[op]  # several rows: measured slower (2,000 rows of 100), left to the chain
            assert d8._route(op, z8, p8[:1]) == d8._route(op, z8[:1], p8) == off8[op]  # a shared row, a shared block: not measured
            assert d8._route(op, z8[:1], p8[:1]) == ("wide_flow_streamed", False, False)
        big = torch.zeros(1, 1, 8).expand(1, (1 << 17) + 1, 8)  # (a view: nothing that large is allocated)
        assert d8._route("log_prob", big[:, :1 << 17], p8[:1]).family == "wide_flow_streamed"
        assert d8._route("log_prob", big, p8[:1]).family == "fused"  # one row of 2^20 samples: measured slower
        assert d8._route("inverse", big[:, :1 << 17], p8[:1]).family == "wide_flow_streamed"
        assert d8._route("forward", big[:, :1 << 12], p8[:1]).family == "wide_flow_streamed"
        assert d8._route("forward", big[:, :(1 << 12) + 1], p8[:1]).family == "fused"  # sampling: a tie at 2^17, won at 2^12
        # every other D: the whole predicate
        nf, p = _flow(6, 5, 2, 20)
        z = torch.zeros(3, 40, 6)
        off = {op: nf._route(op, z, p) for op in ("log_prob", "inverse", "forward")}
        assert all(r.family == "bijectors" for r in off.values())  # the per-bijector composition
        nf.wide_flow_streamed = True
        for op in off:
            assert nf._route(op, z, p) == ("wide_flow_streamed", False, False)
            assert nf._route(op, z, p[:1]) == ("wide_flow_streamed", False, False)  # one shared row
        assert nf._route("forward", z, p[:1], f32_draw=True) == ("wide_flow_streamed", False, False)  # the caller forms log_q
        assert nf._route("log_prob", z[:1], p).family == "wide_flow_streamed"  # one block of z
        assert nf._route("forward", z, p, freeze_bn=False).family != "wide_flow_streamed"  # fresh statistics
        assert nf._route("log_prob", z[:, :31], p).family == "bijectors"  # several rows with N < 32
        assert nf._route("log_prob", z[:, :31], p[:1]).family == "wide_flow_streamed"  # ... but any N with one row
        assert nf._route("log_prob", z[0], p[:1]).family != "wide_flow_streamed"  # 2-d z
        assert nf._route("log_prob", z.double(), p).family == "bijectors"
        nf.fusion = _lib.FUSE_LAYER
        assert nf._route("log_prob", z, p) == off["log_prob"]  # FUSE_LAYER keeps today's route
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("log_prob", z, p).family == "wide_flow_streamed"
        nf.fusion = _lib.FUSE_AUTO
    pg = p.clone().requires_grad_()
    assert nf._route("log_prob", z, pg).family not in ("wide_flow_streamed", "fused")  # autograd keeps today's routes
    assert nf._route("forward", z, pg).family != "wide_flow_streamed"
    assert nf._route("log_prob", z.clone().requires_grad_(), p).family != "wide_flow_streamed"
    assert nf._route("log_prob", z, p).family == "wide_flow_streamed"  # grad mode on, nothing requires grad: plain
    with torch.no_grad():
        ar, pa = _flow(6, 5, 2, 20, arch="AR")
        ar.wide_flow_streamed = True
        assert ar._route("log_prob", z, pa).family == "ar_fused"
        sup, ps = _flow(6, 5, 2, 20, support_layer=tnf.ToInterval(6, [-1.0] * 6, [2.0] * 6))
        sup.wide_flow_streamed = True
        assert sup._route("log_prob", z, ps) == ("wide_flow_streamed", False, False)  # the support layer: its own kernel
        assert sup._route("forward", z, ps[:1]) == ("wide_flow_streamed", False, False)
        assert sup._route("inverse", z, ps).family == "bijectors"
