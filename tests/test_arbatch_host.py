"""Sampling an autoregressive flow with fresh batch statistics as one call each way (include/tnf_arbatch.h), without a
GPU: the closed-form backward (tests/arbatch_restatement.py) against float64 autograd through the oracle's MAF, batch-mode
BatchNorm and Affine; four planted defects against the largest bar the GPU tests can take; header, exports and binding
table in step; the two predicates; every refusal that precedes a launch; the routing of NormFlow with the switch
`ar_batch_forward` off and on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import arbatch_restatement as B
import maf_restatement as MR
import test_route_table as RT

import torch_nf_amd as tnf
from torch_nf_amd import _lib, arbatch_ops

lib = _lib.lib
INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
NAMES = ("tnf_ar_flow_batch_supported", "tnf_ar_flow_batch_train_supported", "tnf_arbatch_launch_count",
         "tnf_ar_flow_forward_batch_workspace_bytes", "tnf_ar_flow_forward_batch_f32",
         "tnf_ar_flow_batch_bwd_workspace_bytes", "tnf_ar_flow_batch_bwd_f32")


# ---- the algorithm, before any kernel ------------------------------------------------------------------------------------
def _inputs(oracle, D, L, U, M, Mp, N, seed):
    rng = np.random.RandomState(seed)
    _, Ms = oracle.maf_masks(D, L, U, True, np.random.RandomState(seed + 1))
    Ms = [np.asarray(m, dtype=np.float64) for m in Ms]
    n = oracle.maf_num_params(D, L, U)
    t = lambda *s: torch.tensor(rng.normal(0, 1, s))  # noqa: E731
    params = torch.cat([t(Mp, n) * 0.3, t(Mp, 2 * D) * 0.4], 1)  # distinct Affine rows when Mp > 1
    return Ms, n, params, t(M, N, D), t(M, N, D), t(M, N)


@pytest.mark.parametrize("folded", [False, True])
@pytest.mark.parametrize("Mp", [1, 3])
@pytest.mark.parametrize("D,L,U", [(2, 1, 15), (5, 1, 20), (6, 2, 15), (8, 3, 16)])
def test_restatement_against_float64_autograd(oracle, D, L, U, Mp, folded):
    """z only, log_q only, both: within 1e-9 of the largest entry.  folded=True is in float64 the same function."""
    M, N = 3, 7
    Ms, n, params, omega, wz, wl = _inputs(oracle, D, L, U, M, Mp, N, seed=10 * D + Mp)
    base = torch.tensor(oracle.base_log_density_f64(omega.numpy()))
    for _, cz, cl in B.LOSSES:
        q = params.clone().requires_grad_()
        x, ld = oracle.maf(omega, q[:, :n], D, L, U, Ms, False)
        y, ld2, mean, alpha = oracle.bn_forward_batch(x.contiguous(), eps=B.EPS)
        z, ld3 = oracle.affine(y, q[:, n:], D, False)
        log_q = base - ld - ld2 - ld3
        (cz * (z * wz).sum() + cl * (log_q * wl).sum()).backward()
        with torch.no_grad():
            z_r, sld_r, mean_r, alpha_r = B.forward(oracle, omega, params, Ms, D, L, U)
            got = B.backward(z_r, params, Ms, mean_r, alpha_r, cz * wz, -cl * wl, D, L, U, folded=folded)
        torch.testing.assert_close(z_r, z.detach(), rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(sld_r, (ld + ld2 + ld3).detach(), rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(mean_r, mean.detach(), rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(alpha_r, alpha.detach(), rtol=1e-10, atol=1e-10)
        assert got.dtype == torch.float64 and MR.gerr(got, q.grad) <= 1e-9, (cz, cl, MR.gerr(got, q.grad))


@pytest.mark.parametrize("shape", [B.TRAIN_SHAPES[0], B.TRAIN_SHAPES[1]], ids=B.shape_id)
def test_planted_defects_exceed_the_gpu_bars(shape):
    """On the GPU test's own inputs (per-context rows and one shared row, M > 1 in both): each defect, in float64, moves
    the gradient of the loss `both` by more than CAP, the largest bar tests/test_gpu_arbatch.py can take."""
    D, L, U = shape[:3]
    pr = B.problem(shape)
    want = pr["want"]["both"]
    args = (pr["z64"], pr["params"].double(), pr["Ms"], pr["mean64"], pr["alpha64"], pr["wz"].double(), -pr["wl"].double(),
            D, L, U)
    assert MR.gerr(B.backward(*args), want) == 0.0
    for defect, part in (("drop_G", 0), ("drop_P", 0), ("context_n", 0), ("drop_gs", 1)):
        got = B.backward(*args, **{defect: True})
        e, blocks = MR.gerr(got, want), B.split_err(got, want, pr["n"])
        print("planted %s on %s: row %.2e (MAF block %.2e, Affine slice %.2e)" % (defect, B.shape_id(shape), e, *blocks))
        assert e > B.CAP and blocks[part] > B.CAP and blocks[1 - part] == 0.0, (defect, e, blocks)
    assert max(pr["noise"].values()) < B.CAP / 4  # the noise model itself is far inside the cap


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_arbatch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.ARBATCH_SIGNATURES) == sorted(NAMES) and len(protos) == 7
    others = set()
    for table in ("SIGNATURES", "MOG_SIGNATURES", "ABC_SIGNATURES", "HEBB_SIGNATURES", "EFN_SIGNATURES",
                  "PADTRAIN_SIGNATURES", "PADBATCH_SIGNATURES", "CTXFLOW_SIGNATURES", "CTXTRAIN_SIGNATURES",
                  "SAMPLETRAIN_SIGNATURES", "ARSAMPLE_SIGNATURES"):
        others |= set(getattr(_lib, table))
    assert not set(_lib.ARBATCH_SIGNATURES) & others  # disjoint from the other eleven
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.ARBATCH_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t, int32_t and float
            want = (ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32 if "int32_t" in p
                    else ctypes.c_float)
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p or "float " in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    for name in ("tnf_arbatch_launch_count", "tnf_ar_flow_forward_batch_workspace_bytes",
                 "tnf_ar_flow_batch_bwd_workspace_bytes"):
        assert _lib.ARBATCH_SIGNATURES[name][0] is ctypes.c_int64
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_arbatch.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+\s*\(", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    assert _lib.DIAG_FAMILIES == 19  # counters of its own: the flow families are a closed set
    assert [arbatch_ops.arbatch_launch_count(w) >= 0 for w in range(4)] == [True] * 4
    assert lib.tnf_arbatch_launch_count(4) == INV and lib.tnf_arbatch_launch_count(-1) == INV


def test_predicates_against_their_definitions():
    ones = [0, 0]
    for D in list(range(1, 35)) + [48, 64, 65]:
        for L in range(1, 7):
            for U in (1, 15, 16, 17, 32, 42, 48, 49, 64, 65):
                fwd, trn = lib.tnf_ar_flow_batch_supported(D, L, U), lib.tnf_ar_flow_batch_train_supported(D, L, U)
                assert fwd == lib.tnf_ar_flow_supported(D, L, U), (D, L, U)
                assert trn == int(fwd == 1 and lib.tnf_maf_sample_bwd_supported(D, L, U) == 1), (D, L, U)
                assert arbatch_ops.ar_flow_batch_supported(D, L, U) == bool(fwd)
                assert arbatch_ops.ar_flow_batch_train_supported(D, L, U) == bool(trn)
                ones[0] += fwd
                ones[1] += trn
    assert ones[0] > ones[1] > 300  # neither vacuous, and the forward's domain is the wider one
    for s in B.TRAIN_SHAPES:
        assert lib.tnf_ar_flow_batch_train_supported(*s[:3]) == 1, s
    for s in B.FORWARD_ONLY:
        assert lib.tnf_ar_flow_batch_supported(*s[:3]) == 1 and lib.tnf_ar_flow_batch_train_supported(*s[:3]) == 0, s
    assert lib.tnf_ar_flow_batch_supported(65, 2, 15) == 0 and lib.tnf_ar_flow_batch_supported(0, 2, 15) == 0
    assert lib.tnf_ar_flow_batch_train_supported(33, 2, 15) == 0 and lib.tnf_ar_flow_batch_train_supported(6, 4, 15) == 0


def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]  # never dereferenced: every call fails validation first
    counts = [arbatch_ops.arbatch_launch_count(w) for w in range(4)]
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]
    D, L, U = 6, 2, 15
    need = lib.tnf_maf_num_params(D, L, U) + 2 * D
    big = 1 << 40

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    def fwd(**kw):
        a = dict(omega=p[0], params=p[1], masks=p[2], z=p[3], sld=p[4], mean=p[5], alpha=p[6], M=3, Mp=3, N=40, D=D, L=L, U=U,
                 pstride=need, eps=1e-5, ws=p[8], ws_bytes=big)
        a.update(kw)
        return lib.tnf_ar_flow_forward_batch_f32(a["omega"], a["params"], a["masks"], a["z"], a["sld"], a["mean"], a["alpha"],
                                                 a["M"], a["Mp"], a["N"], a["D"], a["L"], a["U"], a["pstride"], a["eps"],
                                                 a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(z=p[0], params=p[1], masks=p[2], mean=p[3], alpha=p[4], g_z=p[5], g_sld=p[6], g_params=p[7], M=3, Mp=3,
                 N=40, D=D, L=L, U=U, pstride=need, gpstride=need, ws=p[8], ws_bytes=big)
        a.update(kw)
        return lib.tnf_ar_flow_batch_bwd_f32(a["z"], a["params"], a["masks"], a["mean"], a["alpha"], a["g_z"], a["g_sld"],
                                             a["g_params"], a["M"], a["Mp"], a["N"], a["D"], a["L"], a["U"], a["pstride"],
                                             a["gpstride"], a["ws"], a["ws_bytes"], None)

    for call, tag, ptrs, strides, wsq, unsup in (
            (fwd, b"tnf_ar_flow_forward_batch_f32", ("omega", "params", "masks", "z", "sld", "mean", "alpha"), ("pstride",),
             lib.tnf_ar_flow_forward_batch_workspace_bytes, (dict(D=65), dict(D=0), dict(L=6), dict(L=0), dict(U=65), dict(U=0))),
            (bwd, b"tnf_ar_flow_batch_bwd_f32", ("z", "params", "masks", "mean", "alpha", "g_params"), ("pstride", "gpstride"),
             lib.tnf_ar_flow_batch_bwd_workspace_bytes, (dict(D=33), dict(D=0), dict(L=4), dict(L=0), dict(U=65), dict(U=0)))):
        for name in ptrs:
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in (dict(M=0), dict(M=-3), dict(Mp=2), dict(Mp=0), dict(N=-1), dict(M=1, Mp=3)):
            refused(call(**kw), INV, tag + b": M=")
        for kw in unsup:
            refused(call(**kw), UNSUP, tag + b": no kernel for D=")
        for name in strides:
            refused(call(**{name: need - 1}), INV, tag + b": parameter rows shorter than %d" % need)
        refused(call(M=1, Mp=1, N=1), INV, tag + b": batch statistics need more than one row")
        assert call(M=1, Mp=1, N=2, ws_bytes=0) == WS  # ... two rows pass that check
        assert call(N=0) == 0  # nothing to do: OK, no launch
        refused(call(N=0, pstride=need - 1), INV, tag + b": parameter rows shorter")  # ... after the other checks
        ws_need = wsq(3, 3, 40, D)
        assert ws_need > 0 and ws_need % 16 == 0 and wsq(1, 1, 40, D) <= ws_need
        assert wsq(0, 0, 40, D) == INV and wsq(3, 2, 40, D) == INV and wsq(3, 3, -1, D) == INV and wsq(3, 3, 40, 0) == INV
        for kw in (dict(ws=None), dict(ws_bytes=ws_need - 1), dict(ws_bytes=0), dict(ws=ctypes.c_void_p(4096 + 8))):
            assert call(**kw) == WS and tag in lib.tnf_last_error(), kw
        assert call(ws_bytes=ws_need, N=0) == 0
    refused(fwd(z=p[0]), INV, b"z_out must not alias omega")
    refused(bwd(g_z=None, g_sld=None), INV, b"g_z and g_sld are both NULL")
    refused(bwd(g_params=p[1]), INV, b"g_params must not alias params")
    assert bwd(g_z=None, N=0) == 0 and bwd(g_sld=None, N=0) == 0
    assert lib.tnf_ar_flow_batch_bwd_workspace_bytes(3, 3, 40, 33) == INV
    # the backward's workspace holds the partial sums of every slice of pass 1
    assert lib.tnf_ar_flow_batch_bwd_workspace_bytes(1, 1, 40000, 4) > lib.tnf_ar_flow_batch_bwd_workspace_bytes(1, 1, 40, 4)
    assert [arbatch_ops.arbatch_launch_count(w) for w in range(4)] == counts  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing -------------------------------------------------------------------------------------------------------------
ENTRIES = ("ar_flow_forward_batch_raw", "ar_flow_forward_batch_train")


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.ar_batch_forward` = switch and the new module's entries recorded."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tnf.NormFlow, "ar_batch_forward", switch)
        trace = []
        for name in ENTRIES:
            def recorder(*args, _name=name, **kwargs):
                trace.append(_name)
                raise RT._Reached()

            mp.setattr(arbatch_ops, name, recorder)
        out = RT.run_row(r)
    return out + trace


def _candidates():
    return [r for r in RT.GRID if r["arch"] == "AR" and r["op"] == "forward" and not r["freeze_bn"]]


def test_switch_off_is_todays_route_on_the_fresh_statistics_ar_rows():
    table = RT._table()
    rows = _candidates()
    assert len(rows) > 40
    for r in rows:
        assert run_row(r, False) == table[RT.row_id(r)], RT.row_id(r)


def test_switch_on_changes_hands_only_where_the_families_apply():
    table, taken = RT._table(), {name: 0 for name in ENTRIES}
    for r in RT.GRID:
        if r["arch"] != "AR":
            continue
        old, on = table[RT.row_id(r)], run_row(r, True)
        if on == old:
            continue
        rid = RT.row_id(r)
        assert r in _candidates() and on[-1] in ENTRIES and on[:-1] == old[:1] == ["base_log_density_f64"], rid
        # (a forward row draws omega itself, float32 after staging whatever its zdtype says; float64 parameters are
        # excluded in test_families_and_their_exclusions)
        assert not r["reduce"] and (r["M"] if r["rows"] == "M" else 1) * r["N"] >= 2, rid
        train = on[-1] == ENTRIES[1]
        assert train == (r["p_grad"] and not r["no_grad"]), rid
        assert not (train and r["D"] > 32), rid  # D = 48 under autograd keeps the composition
        taken[on[-1]] += 1
    assert min(taken.values()) >= 3, taken


def test_families_and_their_exclusions():
    assert tnf.NormFlow.ar_batch_forward is False
    nf = tnf.NormFlow(6, True, "AR", 1, 2, 15, device="cpu")
    om, p = torch.zeros(3, 40, 6), torch.zeros(3, nf.D_params, requires_grad=True)
    fresh = lambda z, q, **kw: nf._route("forward", z, q, freeze_bn=False, **kw)  # noqa: E731
    assert fresh(om, p).family == "bijectors"  # the switch defaults to off
    nf.ar_batch_forward = True
    assert fresh(om, p) == ("ar_batch_train", False, False) and fresh(om, p, f32_draw=True) == ("ar_batch_train", False, False)
    assert fresh(om, p.detach()) == ("ar_batch_chain", False, False)  # nothing requires grad: the plain chain
    with torch.no_grad():
        assert fresh(om, p).family == "ar_batch_chain"
    assert fresh(om[:1, :2], p[:1]).family == "ar_batch_train" and fresh(om[:2, :1], p[:2]).family == "ar_batch_train"  # n = 2
    assert fresh(om[:1, :1], p[:1]).family == "bijectors"  # one row has no batch statistics
    big, edge = torch.zeros(1, 26667, 6), torch.zeros(1, 26666, 6)  # M N D = 160,002 and 159,996
    assert fresh(big, p[:1].detach()).family == "bijectors" and fresh(edge, p[:1].detach()).family == "ar_batch_chain"
    assert fresh(big, p[:1]).family == "ar_batch_train"  # the measured tie is the plain chain's alone
    assert fresh(om, p[:1]).family == "bijectors" and fresh(om[:1], p).family == "bijectors"  # one block per parameter row
    assert fresh(om.double(), p.double()).family == "bijectors"  # float64
    assert fresh(om.double(), p.double().detach()).family == "bijectors"
    assert fresh(om[0], p).family == "bijectors"  # 2-d
    assert nf._route("forward", om, p).family != "ar_batch_train"  # frozen statistics: today's routes
    assert nf._route("log_prob", om, p).family == "ar_train"
    from torch_nf_amd import ops
    with pytest.MonkeyPatch.context() as mp:  # the bf16 operand experiment keeps today's route under autograd
        mp.setattr(ops, "current_operand_precision", lambda: "bf16")
        assert fresh(om, p).family == "bijectors"
    nf.batch_stats_reduce = lambda moments: moments  # sample-sharded statistics
    assert fresh(om, p).family == "bijectors" and fresh(om, p.detach()).family == "bijectors"
    nf.batch_stats_reduce = None
    wide = tnf.NormFlow(48, True, "AR", 1, 2, 15, device="cpu")  # D = 48: the chain only
    wide.ar_batch_forward = True
    ow, pw = torch.zeros(1, 8, 48), torch.zeros(1, wide.D_params, requires_grad=True)
    assert wide._route("forward", ow, pw, freeze_bn=False).family == "bijectors"
    assert wide._route("forward", ow, pw.detach(), freeze_bn=False).family == "ar_batch_chain"
    for support in (tnf.ToInterval(6, [-1.0] * 6, [2.0] * 6), tnf.ToSimplex(6)):  # any support layer: its own op behind
        sup = tnf.NormFlow(6, True, "AR", 1, 2, 15, support, device="cpu")
        sup.ar_batch_forward = True
        ps = torch.zeros(1, sup.D_params, requires_grad=True)
        assert sup._route("forward", torch.zeros(1, 8, 6), ps, freeze_bn=False) == ("ar_batch_train", False, False)
    cp = tnf.NormFlow(6, True, "coupling", 2, 2, 15, device="cpu")
    cp.ar_batch_forward = True
    assert not cp._route("forward", om, torch.zeros(3, cp.D_params, requires_grad=True), freeze_bn=False).family.startswith("ar_")
