"""Training coupling flows of width 2 <= D <= 63 through the reversible backward at the embedded width 2H
(include/tnf_padtrain.h), without a GPU: header, exports and binding table in step; the support predicate over its whole
domain; the index map against an independent restatement and -- the claim the feature rests on -- against the float64
oracle: the embedded flow has the log_prob (plus a constant) and the gradients of the real one; every refusal that
precedes a launch; and the routing of NormFlow with the switch `padded_training` on and off."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import test_route_table as RT

import torch_nf_amd as tnf
from torch_nf_amd import _lib, padtrain_ops

lib = _lib.lib
INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
WIDTHS = (2, 3, 5, 16, 31, 33, 47, 63)


def half(D):
    return 16 if D <= 31 else 32


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_padtrain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.PADTRAIN_SIGNATURES) and len(protos) == 10
    others = (set(_lib.SIGNATURES) | set(_lib.MOG_SIGNATURES) | set(_lib.ABC_SIGNATURES) | set(_lib.HEBB_SIGNATURES)
              | set(_lib.EFN_SIGNATURES))
    assert not set(_lib.PADTRAIN_SIGNATURES) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.PADTRAIN_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    header = open(os.path.join(ROOT, "include", "tnf_padtrain.h")).read()
    assert '#include "tnf_padtrain.h"' in open(os.path.join(ROOT, "include", "tnf.h")).read()
    for n in ("EMBED_ROWS", "GATHER_ROWS", "EMBED_PARAMS", "GATHER_PARAMS", "BWD"):
        assert "TNF_PADTRAIN_COUNT_%s = %d" % (n, getattr(_lib, "PADTRAIN_COUNT_" + n)) in header
    assert "TNF_PADTRAIN_COUNTERS = 5" in header
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(5):
        assert lib.tnf_padtrain_launch_count(which) >= 0
    assert lib.tnf_padtrain_launch_count(5) == -1 and b"tnf_padtrain_launch_count" in lib.tnf_last_error()
    assert lib.tnf_padtrain_launch_count(-1) == -1


def test_predicate_is_the_conjunction_over_the_domain():
    assert [lib.tnf_flow_padded_width(D) for D in (-1, 0, 1, 2, 31, 32, 33, 63, 64, 65)] == [0, 0, 0, 32, 32, 0, 64, 64, 0, 0]
    rev = {(W, S, L, U): lib.tnf_flow_train_rev_supported(W, S, L, U)
           for W in (32, 64) for S in range(1, 17) for L in range(1, 5) for U in (15, 16, 17)}
    for D in range(2, 65):
        W = lib.tnf_flow_padded_width(D)
        assert W == (0 if D in (32, 64) else 2 * half(D))
        for S in range(1, 17):
            for L in range(1, 5):
                for U in (15, 16, 17):
                    want = int(bool(W) and lib.tnf_flow_padded_supported(D, S, L, U) == 1 and rev[(W, S, L, U)] == 1)
                    assert lib.tnf_flow_padded_train_supported(D, S, L, U) == want, (D, S, L, U)
    # the largest S: the minimum of the two pinned tables (tests/test_padded_flow_host.py, tests/test_cabi.py)
    s_max = {(16, 1): 14, (16, 2): 8, (16, 3): 6, (32, 1): 6, (32, 2): 4, (32, 3): 3}
    for D in (2, 3, 4, 5, 8, 16, 17, 31, 33, 40, 47, 48, 63):
        for L in (1, 2, 3):
            for U in (15, 16):
                got = [S for S in range(1, 20) if lib.tnf_flow_padded_train_supported(D, S, L, U)]
                assert got == list(range(1, s_max[(half(D), L)] + 1)), (D, L, U, got)
    for D in (1, 32, 64, 0, -3, 65):
        assert lib.tnf_flow_padded_train_supported(D, 1, 1, 15) == 0
    assert lib.tnf_flow_padded_train_supported(5, 1, 4, 15) == 0 and lib.tnf_flow_padded_train_supported(5, 1, 2, 17) == 0
    assert lib.tnf_flow_padded_train_supported(5, 0, 2, 15) == 0
    assert lib.tnf_flow_train_rev_supported(8, 2, 2, 15) == 0  # the existing predicate keeps its value


# ---- the index map --------------------------------------------------------------------------------------------------------
def embed_row(row, D, S, L, U, oracle, fill=0.0):
    """The embedded layout restated with reshapes: one real row (P,) -> the (P',) row of width 2H, `fill` at padding."""
    H, h, out, off = half(D), D // 2, [], 0
    for kind, n, upper in oracle.flow_layout(D, S, L, U):
        if kind == "coupling":
            din, dout = oracle.coupling_dims(D, upper)
            for i, o, I, O in [(din, U, H, U)] + [(U, U, U, U)] * (L - 1) + [(U, dout, U, H)]:
                for _ in range(2):  # W_t, W_s: row-major [in][out]
                    w = np.full((I, O), fill, dtype=row.dtype)
                    w[:i, :o] = row[off:off + i * o].reshape(i, o)
                    out.append(w.ravel())
                    off += i * o
                for _ in range(2):  # b_t, b_s
                    b = np.full(O, fill, dtype=row.dtype)
                    b[:o] = row[off:off + o]
                    out.append(b)
                    off += o
        elif kind == "affine":
            for _ in range(2):  # alpha, shift
                out.append(embed_features(row[off:off + D], D, fill))
                off += D
    assert off == row.shape[0]
    return np.concatenate(out)


def embed_features(x, D, fill=0.0):
    """(..., D) -> (..., 2H): features 0 .. h-1 at the front of the first half, h .. D-1 at the front of the second."""
    H, h = half(D), D // 2
    out = np.full(x.shape[:-1] + (2 * H,), fill, dtype=x.dtype)
    out[..., :h] = x[..., :h]
    out[..., H:H + D - h] = x[..., h:]
    return out


def index_map(D, S, L, U, oracle):
    """real index -> embedded index, from the restatement: embed the row 0 .. P-1 and look where each value went."""
    P = oracle.flow_num_params(D, S, L, U)
    emb = embed_row(np.arange(P, dtype=np.int64), D, S, L, U, oracle, fill=-1)
    assert emb.shape[0] == oracle.flow_num_params(2 * half(D), S, L, U)
    pos = np.nonzero(emb >= 0)[0]
    e = np.empty(P, dtype=np.int64)
    e[emb[pos]] = pos
    return e


@pytest.mark.parametrize("D", WIDTHS)
def test_embed_index_is_the_restated_map(D, oracle):
    for L in (1, 2, 3):
        for U in (15, 16):
            S = 2 if L < 3 else 1
            P, Pe = lib.tnf_flow_num_params(D, S, L, U), lib.tnf_flow_num_params(2 * half(D), S, L, U)
            got = np.array([lib.tnf_flow_padded_embed_index(D, S, L, U, k) for k in range(P)])
            assert got.min() >= 0 and got.max() < Pe  # in range
            assert np.all(np.diff(got) > 0)  # strictly increasing, so injective: padding is the gaps (embed_params)
            np.testing.assert_array_equal(got, index_map(D, S, L, U, oracle))
            for k in (-1, P, P + 7):
                assert lib.tnf_flow_padded_embed_index(D, S, L, U, k) == -1
    assert lib.tnf_flow_padded_embed_index(32, 1, 1, 15, 0) == -1 and lib.tnf_flow_padded_embed_index(64, 1, 1, 15, 0) == -1
    assert lib.tnf_flow_padded_embed_index(D, 0, 1, 15, 0) == -1 and lib.tnf_flow_padded_embed_index(D, 1, 0, 15, 0) == -1


@pytest.mark.parametrize("per_context", [False, True])
@pytest.mark.parametrize("D,S,L,U", [(2, 2, 1, 15), (3, 1, 2, 16), (5, 2, 3, 15), (16, 1, 1, 16), (31, 2, 2, 15),
                                     (33, 1, 3, 16), (47, 2, 1, 15), (63, 1, 2, 16)])
def test_embedded_flow_is_the_real_flow_in_float64(D, S, L, U, per_context, oracle):
    """The claim itself: embed with tnf_flow_padded_embed_index, run the float64 oracle at width 2H -- log_prob differs
    by the constant (2H - D) log sqrt(2 pi), the gradients at the real slots are the real gradients, d z at the padded
    features is exactly 0."""
    W, M, N = 2 * half(D), 2, 5
    Mp = M if per_context else 1
    rng = np.random.RandomState(D)
    P, Pe = lib.tnf_flow_num_params(D, S, L, U), lib.tnf_flow_num_params(W, S, L, U)
    e = torch.tensor([lib.tnf_flow_padded_embed_index(D, S, L, U, k) for k in range(P)])
    p = torch.tensor(rng.normal(0, 0.3, (Mp, P)), requires_grad=True)
    z = torch.tensor(rng.normal(0, 1, (M, N, D)), requires_grad=True)
    mean, alpha = rng.normal(0, 0.3, (2 * S, D)), np.exp(rng.normal(0, 0.2, (2 * S, D)))
    w = torch.tensor(rng.normal(0, 1, (M, N)))
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        lp = oracle.flow_log_prob(z, p, D, S, L, U, [(torch.tensor(m), torch.tensor(a)) for m, a in zip(mean, alpha)])
        (lp * w).sum().backward()
        pe = torch.zeros(Mp, Pe, dtype=torch.float64)
        pe[:, e] = p.detach()
        pe.requires_grad_()
        ze = torch.tensor(embed_features(z.detach().numpy(), D), requires_grad=True)
        stats = [(torch.tensor(m), torch.tensor(a))
                 for m, a in zip(embed_features(mean, D, 0.0), embed_features(alpha, D, 1.0))]
        lpe = oracle.flow_log_prob(ze, pe, W, S, L, U, stats) + (W - D) * math.log(math.sqrt(2.0 * math.pi))
        (lpe * w).sum().backward()
    finally:
        torch.set_default_dtype(before)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lpe, lp, **tol)
    torch.testing.assert_close(pe.grad[:, e], p.grad, **tol)
    real = torch.tensor(embed_features(np.ones(D), D)) > 0
    torch.testing.assert_close(ze.grad[..., real], z.grad, **tol)
    assert bool((ze.grad[..., ~real] == 0).all())
    # ... and the restated layout is that embedding (one row)
    np.testing.assert_array_equal(embed_row(p.detach().numpy()[0], D, S, L, U, oracle), pe.detach().numpy()[0])


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    counts = [lib.tnf_padtrain_launch_count(w) for w in range(5)]
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    for name in ("tnf_flow_padded_embed_rows_f32", "tnf_flow_padded_gather_rows_f32"):
        fn, tag = getattr(lib, name), name.encode()
        refused(fn(None, p[1], 4, 5, None), INV, tag + b": NULL pointer")
        refused(fn(p[0], None, 4, 5, None), INV, tag + b": NULL pointer")
        refused(fn(p[0], p[1], -1, 5, None), INV, tag + b": R=-1")
        for D in (1, 32, 64, 0):
            refused(fn(p[0], p[1], 4, D, None), UNSUP, tag + b": no embedded layout for D=%d" % D)
        assert fn(p[0], p[1], 0, 5, None) == 0
    refused(lib.tnf_flow_padded_embed_rows_f32(p[0], ctypes.c_void_p(4100), 4, 5, None), INV, b"16-byte aligned")
    refused(lib.tnf_flow_padded_gather_rows_f32(ctypes.c_void_p(4104), p[1], 4, 5, None), INV, b"16-byte aligned")
    assert lib.tnf_flow_padded_embed_rows_f32(ctypes.c_void_p(4100), p[1], 0, 5, None) == 0  # the real side: 4 bytes

    P5 = lib.tnf_flow_num_params(5, 2, 2, 15)

    def embed(**kw):
        a = dict(params=p[0], mean=p[1], alpha=p[2], out=p[3], mean_out=p[4], alpha_out=p[5], Mp=3, D=5, S=2, L=2, U=15,
                 pstride=P5)
        a.update(kw)
        return lib.tnf_flow_padded_embed_params_f32(a["params"], a["mean"], a["alpha"], a["out"], a["mean_out"],
                                                    a["alpha_out"], a["Mp"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                                    None)

    def gather(**kw):
        a = dict(g=p[0], out=p[1], Mp=3, D=5, S=2, L=2, U=15, gpstride=P5)
        a.update(kw)
        return lib.tnf_flow_padded_gather_params_f32(a["g"], a["out"], a["Mp"], a["D"], a["S"], a["L"], a["U"],
                                                     a["gpstride"], None)

    for name in ("params", "mean", "alpha", "out", "mean_out", "alpha_out"):
        refused(embed(**{name: None}), INV, b"tnf_flow_padded_embed_params_f32: NULL pointer")
    for name in ("g", "out"):
        refused(gather(**{name: None}), INV, b"tnf_flow_padded_gather_params_f32: NULL pointer")
    unsupported = (dict(D=32), dict(D=64), dict(D=1), dict(S=9), dict(D=33, S=5), dict(L=4), dict(U=17), dict(S=0))
    for kw in unsupported:
        refused(embed(**kw), UNSUP, b"no padded training for D=")
        refused(gather(**kw), UNSUP, b"no padded training for D=")
    refused(embed(Mp=-1), INV, b"M_p=-1")
    refused(gather(Mp=-2), INV, b"M_p=-2")
    refused(embed(pstride=P5 - 1), INV, b"params row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(gather(gpstride=P5 - 1), INV, b"g_out row has %d elements, flow needs %d" % (P5 - 1, P5))
    assert embed(Mp=0) == 0 and gather(Mp=0) == 0

    wsb = lib.tnf_flow_padded_train_workspace_bytes
    for bad in ((0, 1, 8), (3, 2, 8), (3, 0, 8), (3, 3, -1)):
        refused(wsb(bad[0], bad[1], bad[2], 5, 2, 2, 15), INV, b"tnf_flow_padded_train_workspace_bytes: M=")
    for kw in unsupported:
        a = dict(dict(D=5, S=2, L=2, U=15), **kw)
        refused(wsb(3, 1, 8, a["D"], a["S"], a["L"], a["U"]), UNSUP, b"no padded training for D=")
    # the embedded z0 and g_z, two parameter blocks, the statistics, and the workspace of the backward at width 2H
    for (M, Mp, N, D, S, L, U) in ((3, 1, 8, 5, 2, 2, 15), (3, 3, 40, 33, 2, 1, 16), (1, 1, 4097, 63, 4, 2, 15)):
        W = 2 * half(D)
        r256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
        want = (2 * r256(M * N * W * 4) + 2 * r256(Mp * lib.tnf_flow_num_params(W, S, L, U) * 4) + r256(2 * 2 * S * W * 4)
                + lib.tnf_flow_train_rev_workspace_bytes(M, Mp, N, W, S, L, U))
        assert wsb(M, Mp, N, D, S, L, U) == want

    def bwd(**kw):
        a = dict(z0=p[0], params=p[1], mean=p[2], alpha=p[3], g=p[4], gz=p[5], gp=p[6], M=3, Mp=1, N=8, D=5, S=2, L=2, U=15,
                 pstride=P5, gpstride=P5, ws=p[7], ws_bytes=1 << 40, flag=None)
        a.update(kw)
        return lib.tnf_flow_padded_log_prob_bwd_f32(a["z0"], a["params"], a["mean"], a["alpha"], a["g"], a["gz"], a["gp"],
                                                    a["M"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                                    a["gpstride"], a["ws"], a["ws_bytes"], a["flag"], None)

    tag = b"tnf_flow_padded_log_prob_bwd_f32"
    for name in ("z0", "params", "mean", "alpha", "g", "gp"):
        refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
    for kw in (dict(M=0), dict(Mp=2), dict(Mp=0), dict(N=-1)):
        refused(bwd(**kw), INV, tag + b": M=")
    for kw in unsupported:
        refused(bwd(**kw), UNSUP, tag + b": no padded training for D=")
    refused(bwd(pstride=P5 - 1), INV, tag + b": params row has")
    refused(bwd(gpstride=P5 - 1), INV, tag + b": g_params row too short")
    need = wsb(3, 1, 8, 5, 2, 2, 15)
    refused(bwd(ws_bytes=need - 1), WS, tag + b": workspace %d < %d" % (need - 1, need))
    refused(bwd(ws=None), WS, tag + b": workspace")
    refused(bwd(ws=ctypes.c_void_p(4100)), INV, b"16-byte aligned")
    assert bwd(N=0, ws=None, ws_bytes=0) == 0  # nothing to do: OK, no launch
    assert [lib.tnf_padtrain_launch_count(w) for w in range(5)] == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing: the method of tests/test_route_table.py, with the new entry recorded too -------------------------------------
ENTRY = "flow_padded_log_prob_train"


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.padded_training` = switch (None: the attribute absent, as on a fresh flow)
    and the new ops entry recorded."""
    with pytest.MonkeyPatch.context() as mp:
        if switch is not None:
            mp.setattr(tnf.NormFlow, "padded_training", switch, raising=False)
        trace = []

        def recorder(*args, **kwargs):
            trace.append(ENTRY)
            raise RT._Reached()

        mp.setattr(padtrain_ops, ENTRY, recorder)
        out = RT.run_row(r)
    return out + trace  # the recorder ends the call: its entry is the last one


def takes_padded(r):
    """The conditions of the `train_padded` row of the routing docstring, from the grid row alone."""
    needs_grad = not r["no_grad"] and (r["p_grad"] or r["z_grad"])
    Mp = r["M"] if r["rows"] == "M" else 1
    return (r["op"] == "log_prob" and r["arch"] == "coupling" and needs_grad and r["zdtype"] == "float32"
            and not r["stats_graph"] and r["zdim"] == 3 and (Mp == 1 or r["N"] >= 32) and r["fusion"] != "LAYER"
            and r["sup"] != "simplex" and lib.tnf_flow_padded_train_supported(r["D"], r["S"], RT.L, r["U"]) == 1)


LOG_PROB_ROWS = [r for r in RT.GRID if r["op"] == "log_prob" and r["arch"] == "coupling"]


def test_family_is_train_padded_with_the_switch_on():
    for D in (2, 5, 16, 33, 48):
        for S in (1, 4):
            r = RT.row(D=D, S=S, p_grad=True)
            assert RT.row_id(r) in RT._table()  # the rows the recorded table pins
            assert run_row(r, True) == [ENTRY], (D, S)
            assert run_row(r, False) == RT._table()[RT.row_id(r)] == run_row(r, None)
    # z requires grad too; per-context rows with 32 samples each; a ToInterval layer stays its own kernel in front
    assert run_row(RT.row(D=5, z_grad=True, p_grad=True), True) == [ENTRY]
    assert run_row(RT.row(D=5, z_grad=True), True) == [ENTRY]
    assert run_row(RT.row(D=5, p_grad=True, M=3, N=32, rows="M"), True) == [ENTRY]
    assert run_row(RT.row(D=5, p_grad=True, M=3, N=31), True) == [ENTRY]  # one shared row: any N
    assert run_row(RT.row(D=5, p_grad=True, sup="interval"), True) == ["to_interval", ENTRY]
    assert run_row(RT.row(D=5, p_grad=True, fusion="FLOW"), True) == [ENTRY]


@pytest.mark.parametrize("kw", [dict(zdtype="float64"), dict(stats_graph=True), dict(M=3, N=31, rows="M"),
                                dict(fusion="LAYER"), dict(D=64), dict(D=32), dict(U=20), dict(no_grad=True), dict(zdim=2)],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_exclusions_take_the_old_route(kw):
    r = RT.row(**dict(dict(D=5, p_grad=True), **kw))
    assert RT.row_id(r) in RT._table()
    assert run_row(r, True) == RT._table()[RT.row_id(r)]
    assert ENTRY not in run_row(r, True)


def test_every_log_prob_row_of_the_grid_on_and_off():
    """Switch off (or absent): every route of the recorded table is unchanged.  Switch on: a row changes exactly when the
    conditions of the new family hold, and then only in its last entry -- the kernel entry that the call reaches."""
    table, changed = RT._table(), 0
    for r in LOG_PROB_ROWS:
        old = table[RT.row_id(r)]
        assert run_row(r, False) == old, RT.row_id(r)
        on = run_row(r, True)
        if takes_padded(r) and not old[-1].startswith("raises"):
            assert on == old[:-1] + [ENTRY], RT.row_id(r)
            changed += 1
        else:
            assert on == old, RT.row_id(r)
    assert changed >= 20
    for r in RT.GRID[::7]:  # the other operations and architectures never ask
        if r not in LOG_PROB_ROWS:
            assert run_row(r, True) == table[RT.row_id(r)], RT.row_id(r)


def test_train_path_evaluated_once_per_call_with_the_switch_on(monkeypatch):
    calls = []
    real = tnf.NormFlow._train_path
    monkeypatch.setattr(tnf.NormFlow, "_train_path", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for r in LOG_PROB_ROWS:
        del calls[:]
        run_row(r, True)
        assert len(calls) <= 1, (RT.row_id(r), len(calls))


def test_switch_defaults_to_off_and_names_the_pair():
    nf = tnf.NormFlow(5, True, "coupling", 2, 2, 15, device="cpu")
    assert getattr(nf, "padded_training", False) is False
    z, p = torch.zeros(1, 64, 5), torch.zeros(1, nf.D_params, requires_grad=True)
    assert nf._train_path(z, p) is None  # width 5 has no fused training pair without the switch
    nf.padded_training = True
    assert nf._train_path(z, p) == "padded"
    nf.fusion = _lib.FUSE_LAYER
    assert nf._train_path(z, p) is None
    nf.fusion = _lib.FUSE_AUTO
    assert nf._train_path(torch.zeros(3, 31, 5), torch.zeros(3, nf.D_params)) is None
    assert nf._train_path(torch.zeros(3, 32, 5), torch.zeros(3, nf.D_params)) == "padded"
    assert padtrain_ops.padded_width(5) == 32 and padtrain_ops.padded_width(47) == 64
