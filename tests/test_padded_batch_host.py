"""Sampling coupling flows of width 2 <= D <= 63 with fresh batch statistics through the chains at the embedded width
(include/tnf_padbatch.h), without a GPU: header, exports and binding table in step; the support predicate over a grid
against its definition; every refusal that precedes a launch; the claim the feature rests on -- the embedded chain with
BatchNorm on the real columns only IS the flow of width D -- in float64 against the oracle; and the routing of NormFlow
with the switch `padded_batch_forward` on and off."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import padbatch_restatement as PB
import test_route_table as RT

import torch_nf_amd as tnf
from torch_nf_amd import _lib, padbatch_ops

lib = _lib.lib
INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
COUNTERS = ("FOLD", "GATHER_STATS", "FORWARD", "TRAIN_FWD", "TRAIN_BWD")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_padbatch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.PADBATCH_SIGNATURES) and len(protos) == 8
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES) | set(_lib.PADTRAIN_SIGNATURES))
    assert not set(_lib.PADBATCH_SIGNATURES) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.PADBATCH_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t, int32_t and float
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_float if "float" in p
                    else ctypes.c_int32)
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p or "float" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "tnf_padbatch.h")).read()
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_padbatch.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    for i, n in enumerate(COUNTERS):
        assert "TNF_PADBATCH_COUNT_%s = %d" % (n, i) in header
    assert "TNF_PADBATCH_COUNTERS = 5" in header
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(5):
        assert lib.tnf_padbatch_launch_count(which) >= 0
    assert lib.tnf_padbatch_launch_count(5) == -1 and b"tnf_padbatch_launch_count" in lib.tnf_last_error()
    assert lib.tnf_padbatch_launch_count(-1) == -1


def test_predicate_is_its_definition_over_the_grid():
    """1 exactly when an embedded width exists and the existing chains accept (2H, S, L, U) -- asked of them the way
    NormFlow._batch_chain_ok asks (ops.flow_train_supported at N = 32)."""
    ones = 0
    for D in range(-1, 67):
        W = lib.tnf_flow_padded_width(D)
        for S in (0, 1, 2, 4, 9, 17):
            for L in range(0, 6):
                for U in (0, 1, 15, 16, 17, 20):
                    chains = W != 0 and lib.tnf_flow_train_workspace_bytes(1, 1, 32, W, S, L, U) >= 0
                    assert lib.tnf_flow_padded_batch_supported(D, S, L, U) == int(chains), (D, S, L, U)
                    assert padbatch_ops.flow_padded_batch_supported(D, S, L, U) == chains
                    ones += chains
    assert ones == 61 * 5 * 3 * 3  # D = 2 .. 63 but 32; S >= 1; L = 1 .. 3; U = 1, 15, 16
    for D in (32, 64, 1, 0, 65):
        assert lib.tnf_flow_padded_batch_supported(D, 1, 1, 15) == 0
    assert lib.tnf_flow_padded_batch_supported(5, 17, 3, 16) == 1  # no bound on S: the chains are one launch per layer


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]  # never dereferenced: every call fails validation first
    counts = [lib.tnf_padbatch_launch_count(w) for w in range(5)]
    pt_counts = [lib.tnf_padtrain_launch_count(w) for w in range(5)]
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 15)
    unsupported = (dict(D=32), dict(D=64), dict(D=1), dict(D=65), dict(L=4), dict(L=0), dict(U=17), dict(S=0))
    bad_batch = (dict(M=0), dict(Mp=2), dict(Mp=0), dict(N=-1))

    def forward(**kw):
        a = dict(omega=p[0], params=p[1], z=p[2], sld=p[3], mean=p[4], alpha=p[5], M=3, Mp=1, N=8, D=5, S=2, L=2, U=15,
                 pstride=P5, eps=1e-5, ws=p[6], ws_bytes=1 << 40)
        a.update(kw)
        return lib.tnf_flow_padded_forward_batch_f32(a["omega"], a["params"], a["z"], a["sld"], a["mean"], a["alpha"],
                                                     a["M"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                                     a["eps"], a["ws"], a["ws_bytes"], None)

    def train_fwd(**kw):
        a = dict(omega=p[0], params=p[1], z=p[2], sld=p[3], states=p[7], folds=p[8], mean=p[4], alpha=p[5], M=3, Mp=1, N=8,
                 D=5, S=2, L=2, U=15, pstride=P5, eps=1e-5, ws=p[6], ws_bytes=1 << 40)
        a.update(kw)
        return lib.tnf_flow_padded_forward_train_fwd_f32(a["omega"], a["params"], a["z"], a["sld"], a["states"], a["folds"],
                                                         a["mean"], a["alpha"], a["M"], a["Mp"], a["N"], a["D"], a["S"],
                                                         a["L"], a["U"], a["pstride"], a["eps"], a["ws"], a["ws_bytes"], None)

    def train_bwd(**kw):
        a = dict(omega=p[0], params=p[1], states=p[7], folds=p[8], mean=p[4], alpha=p[5], gz=p[2], gs=p[3], go=p[9],
                 gp=p[6], M=3, Mp=1, N=8, D=5, S=2, L=2, U=15, pstride=P5, gpstride=P5, ws=p[6], ws_bytes=1 << 40)
        a.update(kw)
        return lib.tnf_flow_padded_forward_train_bwd_f32(a["omega"], a["params"], a["states"], a["folds"], a["mean"],
                                                         a["alpha"], a["gz"], a["gs"], a["go"], a["gp"], a["M"], a["Mp"],
                                                         a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], a["gpstride"],
                                                         a["ws"], a["ws_bytes"], None)

    wsb, wsb_train = lib.tnf_flow_padded_batch_workspace_bytes, lib.tnf_flow_padded_batch_train_workspace_bytes
    entries = ((forward, b"tnf_flow_padded_forward_batch_f32", ("omega", "params", "z", "sld", "mean", "alpha"), wsb),
               (train_fwd, b"tnf_flow_padded_forward_train_fwd_f32",
                ("omega", "params", "z", "sld", "states", "folds", "mean", "alpha"), wsb_train),
               (train_bwd, b"tnf_flow_padded_forward_train_bwd_f32",
                ("omega", "params", "states", "folds", "mean", "alpha", "gz", "gs", "gp"), wsb_train))
    for call, tag, pointers, query in entries:
        for name in pointers:
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in bad_batch:
            refused(call(**kw), INV, tag + b": M=")
        refused(call(M=1, N=1), INV, tag + b": batch statistics need more than one row")
        for kw in unsupported:
            refused(call(**kw), UNSUP, tag + b": no padded batch-statistics chain for D=")
        refused(call(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
        need = query(3, 1, 8, 5, 2, 2, 15)
        refused(call(ws_bytes=need - 1), WS, tag + b": workspace %d < %d" % (need - 1, need))
        refused(call(ws=None), WS, tag + b": workspace")
        refused(call(ws=ctypes.c_void_p(4096 + 128)), WS, tag + b": the workspace must be 256-byte aligned")
        assert call(N=0, ws=None, ws_bytes=0) == 0  # nothing to do: OK, no launch
    refused(forward(z=p[0]), INV, b"z_out must not alias omega")
    refused(train_fwd(states=ctypes.c_void_p(4100)), INV, b"states must be 16-byte aligned")
    refused(train_bwd(states=ctypes.c_void_p(4100)), INV, b"states must be 16-byte aligned")
    refused(train_bwd(gpstride=P5 - 1), INV, b"g_params row too short")
    assert train_bwd(go=None, N=0) == 0  # g_omega is optional

    for query, tag in ((wsb, b"tnf_flow_padded_batch_workspace_bytes"), (wsb_train, b"tnf_flow_padded_batch_train_workspace_bytes")):
        for kw in bad_batch:
            a = dict(dict(M=3, Mp=1, N=8), **kw)
            refused(query(a["M"], a["Mp"], a["N"], 5, 2, 2, 15), INV, tag + b": M=")
        for kw in unsupported:
            a = dict(dict(D=5, S=2, L=2, U=15), **kw)
            refused(query(3, 1, 8, a["D"], a["S"], a["L"], a["U"]), UNSUP, tag + b": no padded batch-statistics chain")
    # the embedded rows (omega, z; training: a third block), parameter rows (training: two), statistics, the chain's own
    r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    for (M, Mp, N, D, S, L, U) in ((3, 1, 8, 5, 2, 2, 15), (3, 3, 40, 33, 2, 1, 16), (1, 1, 4097, 63, 4, 3, 15)):
        W = lib.tnf_flow_padded_width(D)
        rows, prow = r256(M * N * W * 4), r256(Mp * lib.tnf_flow_num_params(W, S, L, U) * 4)
        stats = r256(2 * 2 * S * W * 4)
        assert wsb(M, Mp, N, D, S, L, U) == 2 * rows + prow + stats + r256(lib.tnf_flow_forward_batch_workspace_bytes(Mp, W, S, L))
        assert wsb_train(M, Mp, N, D, S, L, U) == (3 * rows + 2 * prow + stats
                                                   + r256(lib.tnf_flow_forward_train_workspace_bytes(M, Mp, N, W, S, L)))

    def fold(**kw):
        a = dict(params=p[0], moments=p[1], mean=p[2], alpha=p[3], fold=p[4], ldc=p[5], Mp=2, D=5, pstride=4000,
                 affine_off=3000, has_affine=1, first=1)
        a.update(kw)
        return lib.tnf_flow_padded_batch_fold_f32(a["params"], a["moments"], a["mean"], a["alpha"], a["fold"], a["ldc"],
                                                  a["Mp"], a["D"], a["pstride"], a["affine_off"], a["has_affine"], a["first"],
                                                  1e-5, None)

    tag = b"tnf_flow_padded_batch_fold_f32"
    for name in ("params", "moments", "mean", "alpha", "fold", "ldc"):
        refused(fold(**{name: None}), INV, tag + b": NULL pointer")
    refused(fold(Mp=0), INV, tag + b": M_p=0")
    for D in (32, 64, 1, 0):
        refused(fold(D=D), UNSUP, tag + b": no embedded layout for D=%d" % D)
    refused(fold(moments=ctypes.c_void_p(4100)), INV, tag + b": moments must be 8-byte aligned")
    refused(fold(affine_off=-1), INV, tag + b": affine_off=-1")
    refused(fold(pstride=3000 + 63), INV, tag + b": affine_off=3000 pstride=3063")  # [alpha (32) | shift (32)] must fit
    assert [lib.tnf_padbatch_launch_count(w) for w in range(5)] == counts  # nothing was launched
    assert [lib.tnf_padtrain_launch_count(w) for w in range(5)] == pt_counts
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- the identity, in float64 on the CPU ------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-5, 0.0])
@pytest.mark.parametrize("D,S,L,U,per_context", [(2, 2, 1, 15, False), (5, 2, 3, 15, True), (16, 1, 1, 16, False),
                                                 (31, 2, 2, 15, True), (33, 1, 3, 16, False), (63, 1, 2, 16, True)])
def test_embedded_chain_is_the_real_flow_in_float64(D, S, L, U, per_context, eps, oracle):
    """oracle coupling / Affine layers at width 2H on embedded inputs, the oracle's BatchNorm on the real columns only:
    z, log_q and every layer's statistics are those of oracle.flow_forward at width D to 1e-12, and the padding is
    exactly 0 after every layer -- also with BatchNorm(eps=0), where sqrt(0 + eps) at a padded column would be 0."""
    M, N = 2, 7
    rng = np.random.RandomState(100 + D)
    P = oracle.flow_num_params(D, S, L, U)
    params = torch.tensor(rng.normal(0, 0.3, (M if per_context else 1, P)))
    omega = rng.normal(0, 1, (M, N, D))
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        z, log_q, stats = PB.flow_forward_eps(omega, params, D, S, L, U, eps, oracle)
        if eps == 1e-5:  # the oracle's own eps: the restated loop is oracle.flow_forward itself
            z_o, log_q_o, stats_o = oracle.flow_forward(omega, params, D, S, L, U)
            assert torch.equal(z, z_o) and torch.equal(log_q, log_q_o)
            assert all(torch.equal(a, b) for s, so in zip(stats, stats_o) for a, b in zip(s, so))
        ze, log_qe, stats_e, z_emb = PB.padded_flow_forward(omega, params, D, S, L, U, eps, oracle)
    finally:
        torch.set_default_dtype(before)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ze, z, **tol)
    torch.testing.assert_close(log_qe, log_q, **tol)
    assert len(stats_e) == len(stats) == 2 * S
    for (m_e, a_e), (m, a) in zip(stats_e, stats):
        assert m_e.shape == (D,) and a_e.shape == (D,)
        torch.testing.assert_close(m_e, m, **tol)
        torch.testing.assert_close(a_e, a, **tol)
    assert bool((z_emb[..., ~PB.real_mask(D)] == 0).all()) and bool(torch.isfinite(z_emb).all())


# ---- routing: the method of tests/test_route_table.py, with the new entries recorded too ---------------------------------
CHAIN, TRAIN = "flow_padded_forward_batch_raw", "flow_padded_forward_train"


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.padded_batch_forward` = switch (None: the attribute absent, as on a fresh
    flow) and the two new ops entries recorded."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is not None:
            mp.setattr(tnf.NormFlow, "padded_batch_forward", switch, raising=False)
        trace = []
        for name in (CHAIN, TRAIN):
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(padbatch_ops, name, recorder)
        out = RT.run_row(r)
    return out + trace  # a recorder ends the call: its entry is the last one


def takes_padded(r):
    """The conditions of the two new rows of the routing docstring, from the grid row alone -> CHAIN, TRAIN or None.
    (The grid draws omega with the parameters' leading dimension, float32 on the device whatever `zdtype` and `z_grad`
    say: those columns shape z of the other operations.  Its parameters are float32.)"""
    if not (r["op"] == "forward" and not r["freeze_bn"] and r["arch"] == "coupling" and not r["reduce"]
            and r["fusion"] != "LAYER" and lib.tnf_flow_padded_batch_supported(r["D"], r["S"], RT.L, r["U"]) == 1):
        return None
    Mp = r["M"] if r["rows"] == "M" else 1
    rows = Mp * r["N"]
    plain = r["no_grad"] or not r["p_grad"]
    inference = plain and not (r["stats_graph"] and not r["no_grad"]) and not (Mp > 1 and r["N"] < 32)
    if rows < 2:
        return None
    return CHAIN if inference else TRAIN if rows >= 32 else None


FRESH_ROWS = [r for r in RT.GRID if r["op"] == "forward" and not r["freeze_bn"]]


def test_families_with_the_switch_on():
    for D in (2, 5, 16, 33, 48):
        for S in (1, 4):
            for kw, entry in ((dict(no_grad=True), CHAIN), (dict(p_grad=True), TRAIN)):
                r = RT.row(op="forward", freeze_bn=False, D=D, S=S, **kw)
                old = RT._table()[RT.row_id(r)]  # the rows the recorded table pins
                assert old == ["base_log_density_f64", "coupling"]
                assert run_row(r, True) == ["base_log_density_f64", entry], (D, S, kw)
                assert run_row(r, False) == old == run_row(r, None)
    fresh = dict(op="forward", freeze_bn=False, D=5)
    # nothing requires grad with grad mode on: inference; per-context rows; a support layer stays its own kernel behind
    assert run_row(RT.row(**fresh), True)[-1] == CHAIN
    assert run_row(RT.row(no_grad=True, M=3, N=32, rows="M", **fresh), True)[-1] == CHAIN
    assert run_row(RT.row(p_grad=True, M=3, N=32, rows="M", **fresh), True)[-1] == TRAIN
    assert run_row(RT.row(p_grad=True, M=3, N=31, rows="M", **fresh), True)[-1] == TRAIN  # 93 rows in the batch
    assert run_row(RT.row(no_grad=True, M=3, N=31, rows="M", **fresh), True)[-1] == TRAIN  # few samples per context
    assert run_row(RT.row(no_grad=True, fusion="FLOW", **fresh), True)[-1] == CHAIN
    assert run_row(RT.row(no_grad=True, draw="torch32", **fresh), True)[-1] == CHAIN
    for sup in ("interval", "simplex"):
        assert run_row(RT.row(no_grad=True, sup=sup, **fresh), True)[-1] == CHAIN
        assert run_row(RT.row(p_grad=True, sup=sup, **fresh), True)[-1] == TRAIN


@pytest.mark.parametrize("kw", [dict(reduce=True), dict(fusion="LAYER"), dict(U=20), dict(D=32), dict(D=64),
                                dict(arch="AR", S=1), dict(freeze_bn=True), dict(M=1, N=1), dict(arch="affine", S=1)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
@pytest.mark.parametrize("grad", [dict(no_grad=True), dict(p_grad=True)], ids=["no_grad", "p_grad"])
def test_exclusions_take_the_old_route(kw, grad):
    r = RT.row(**dict(dict(op="forward", freeze_bn=False, D=5, **grad), **kw))
    assert RT.row_id(r) in RT._table()
    on = run_row(r, True)
    assert on == RT._table()[RT.row_id(r)]
    assert CHAIN not in on and TRAIN not in on


def test_float64_parameters_and_few_rows_are_excluded():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    nf.padded_batch_forward = True
    z = torch.zeros(1, 64, 5)
    with torch.no_grad():
        assert nf._route("forward", z, torch.zeros(1, nf.D_params), freeze_bn=False).family == "batch_chain_padded"
        assert nf._route("forward", z, torch.zeros(1, nf.D_params, dtype=torch.float64), freeze_bn=False).family == "bijectors"
        assert nf._route("forward", z[:, :1], torch.zeros(1, nf.D_params), freeze_bn=False).family == "bijectors"
        assert nf._route("forward", z, torch.zeros(1, nf.D_params), freeze_bn=True).family == "padded"
    p = torch.zeros(1, nf.D_params, requires_grad=True)
    assert nf._route("forward", z, p, freeze_bn=False).family == "batch_train_padded"
    assert nf._route("forward", z[:, :31], p, freeze_bn=False).family == "bijectors"  # fewer than 32 rows under autograd
    assert nf._route("forward", z, p.double(), freeze_bn=False).family == "bijectors"
    assert nf._route("forward", torch.zeros(3, 64, 5), p, freeze_bn=False).family == "bijectors"  # not a row per z row
    nf.padded_batch_forward = False
    assert nf._route("forward", z, p, freeze_bn=False).family == "bijectors"


def test_every_row_of_the_grid_on_and_off():
    """Switch off (or absent): every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of a new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), {CHAIN: 0, TRAIN: 0}
    for r in FRESH_ROWS:
        old = table[RT.row_id(r)]
        assert run_row(r, False) == old, RT.row_id(r)
        on, want = run_row(r, True), takes_padded(r)
        if want is not None and not old[-1].startswith("raises"):
            assert on == old[:-1] + [want], RT.row_id(r)
            changed[want] += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed[CHAIN] >= 20 and changed[TRAIN] >= 20, changed
    for r in RT.GRID[::5]:  # the other operations never ask
        if r not in FRESH_ROWS:
            assert run_row(r, True) == table[RT.row_id(r)], RT.row_id(r)
            assert run_row(r, None) == table[RT.row_id(r)], RT.row_id(r)


def test_switch_defaults_to_off():
    nf = tnf.NormFlow(4, True, "coupling", 1, 1, 15, tnf.ToSimplex(4), device="cpu")
    assert getattr(nf, "padded_batch_forward", False) is False
    assert not nf._padded_batch_ok(torch.zeros(8, 16, 4), torch.zeros(8, nf.D_params))
    nf.padded_batch_forward = True
    assert nf._padded_batch_ok(torch.zeros(8, 16, 4), torch.zeros(8, nf.D_params))
    assert not nf._padded_batch_ok(torch.zeros(8, 16, 4), torch.zeros(1, nf.D_params))
    nf.batch_stats_reduce = lambda m: m
    assert not nf._padded_batch_ok(torch.zeros(8, 16, 4), torch.zeros(8, nf.D_params))
