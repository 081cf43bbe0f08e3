"""Training an autoregressive flow through its samples in one backward kernel (include/tnf_arsample.h), without a GPU:
the kernel's algorithm (tests/arsample_restatement.py) against float64 autograd through the oracle, with the proof that
D - 1 sweeps are exact; header, exports and binding table in step; the support predicate; every refusal that precedes a
launch; the routing of NormFlow with the switch `ar_sample_training` off and on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import arsample_restatement as R
import maf_restatement as MR
import test_route_table as RT

import torch_nf_amd as tnf
from torch_nf_amd import _lib, arsample_ops

lib = _lib.lib
INV, UNSUP, WS = -1, -2, -4  # TNF_EINVAL, TNF_EUNSUPPORTED, TNF_EWORKSPACE
NAMES = ("tnf_maf_sample_bwd_supported", "tnf_arsample_launch_count", "tnf_maf_sample_bwd_f32",
         "tnf_ar_flow_sample_bwd_workspace_bytes", "tnf_ar_flow_sample_bwd_f32")
TOL64 = dict(rtol=1e-9, atol=1e-9)  # the bar test_maf_sampling_direction_backward holds float64 to


# ---- the algorithm, before any kernel ------------------------------------------------------------------------------------
def problem(oracle, D, L, U, M, Mp, N, seed):
    rng = np.random.RandomState(seed)
    _, Ms = oracle.maf_masks(D, L, U, True, np.random.RandomState(seed + 1))
    Ms = [np.asarray(m, dtype=np.float64) for m in Ms]
    n = oracle.maf_num_params(D, L, U)
    t = lambda *s: torch.tensor(rng.normal(0, 1, s))  # noqa: E731
    return dict(Ms=Ms, n=n, p=t(Mp, n + 2 * D) * 0.3, omega=t(M, N, D), wz=t(M, N, D), wl=t(M, N),
                mean=t(D) * 0.3, alpha=torch.tensor(rng.uniform(0.5, 1.5, (D,))))


@pytest.mark.parametrize("Mp", [1, 2])
@pytest.mark.parametrize("D,L,U", [(2, 1, 15), (5, 1, 20), (6, 2, 15), (8, 3, 16)])
def test_restatement_against_float64_autograd(oracle, D, L, U, Mp):
    M, N = 2, 7
    pr = problem(oracle, D, L, U, M, Mp, N, seed=10 * D + Mp)
    Ms, n = pr["Ms"], pr["n"]
    for cz, cl in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):  # both cotangents, and each one alone
        g_x, g_ld = cz * pr["wz"], cl * pr["wl"]
        # the bijector: autograd through the D - 1 passes of oracle.maf(..., inverse=False)
        p, om = pr["p"][:, :n].clone().requires_grad_(), pr["omega"].clone().requires_grad_()
        x, ld = oracle.maf(om, p, D, L, U, Ms, False)
        ((x * g_x).sum() + (ld * g_ld).sum()).backward()
        g_om, g_p, trail = R.maf_sample_bwd(x.detach(), p.detach(), Ms, g_x, g_ld, D, L, U)
        assert len(trail) == D - 1
        torch.testing.assert_close(g_om, om.grad, **TOL64)
        torch.testing.assert_close(g_p, p.grad, **TOL64)
        # N is strictly triangular and its last column is zero: sweep D changes v by exactly 0
        _, _, longer = R.maf_sample_bwd(x.detach(), p.detach(), Ms, g_x, g_ld, D, L, U, sweeps=D)
        last = trail[-1] if trail else torch.exp(oracle._maf_net(x.detach(), p.detach(), D, L, U, Ms)[1]) * g_x
        assert float((longer[-1] - last).abs().max()) == 0.0
        # the stack with frozen statistics: what oracle.ar_flow_forward(..., bn_stat=frozen) composes, in float64
        # (that function itself casts the draw to float32), log_q = base - sum of the log-dets
        q = pr["p"].clone().requires_grad_()
        x, ld = oracle.maf(pr["omega"], q[:, :n], D, L, U, Ms, False)
        y, ld2 = oracle.bn_forward_frozen(x, pr["mean"], pr["alpha"])
        z, ld3 = oracle.affine(y, q[:, n:], D, False)
        sld = ld + ld2 + ld3
        ((z * g_x).sum() + (sld * g_ld).sum()).backward()
        got = R.ar_flow_sample_bwd(z.detach(), q.detach(), Ms, pr["mean"], pr["alpha"], g_x, g_ld, D, L, U)
        torch.testing.assert_close(got, q.grad, **TOL64)


@pytest.mark.parametrize("Mp", [1, 2])
@pytest.mark.parametrize("D,L,U", [(2, 1, 15), (5, 1, 20), (6, 2, 15), (8, 3, 16)])
def test_folded_restatement_against_float64_autograd(oracle, D, L, U, Mp):
    """folded=True -- r = 1 / (1 + 2^a), folded weights, column-sum seeds, alpha in log2 units, h = 1 - 2 r,
    tanh' = 4 r (1 - r) -- is in float64 the same function: bijector and stack, both cotangents and each alone."""
    M, N = 2, 7
    pr = problem(oracle, D, L, U, M, Mp, N, seed=10 * D + Mp)
    Ms, n = pr["Ms"], pr["n"]
    for cz, cl in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
        g_x, g_ld = cz * pr["wz"], cl * pr["wl"]
        p, om = pr["p"][:, :n].clone().requires_grad_(), pr["omega"].clone().requires_grad_()
        x, ld = oracle.maf(om, p, D, L, U, Ms, False)
        ((x * g_x).sum() + (ld * g_ld).sum()).backward()
        g_om, g_p, trail = R.maf_sample_bwd(x.detach(), p.detach(), Ms, g_x, g_ld, D, L, U, folded=True)
        assert len(trail) == D - 1 and g_om.dtype == g_p.dtype == torch.float64
        torch.testing.assert_close(g_om, om.grad, **TOL64)
        torch.testing.assert_close(g_p, p.grad, **TOL64)
        q = pr["p"].clone().requires_grad_()
        x, ld = oracle.maf(pr["omega"], q[:, :n], D, L, U, Ms, False)
        y, ld2 = oracle.bn_forward_frozen(x, pr["mean"], pr["alpha"])
        z, ld3 = oracle.affine(y, q[:, n:], D, False)
        ((z * g_x).sum() + ((ld + ld2 + ld3) * g_ld).sum()).backward()
        got = R.ar_flow_sample_bwd(z.detach(), q.detach(), Ms, pr["mean"], pr["alpha"], g_x, g_ld, D, L, U, folded=True)
        torch.testing.assert_close(got, q.grad, **TOL64)
    if Mp == 1:  # 16-row tiles added in tile order (the long-row variant): the same sums
        om1, wz1, wl1 = (pr[k][:1].repeat(1, 5, *([1] * (pr[k].dim() - 2))) for k in ("omega", "wz", "wl"))
        x = oracle.maf(om1, pr["p"][:, :n], D, L, U, Ms, False)[0]
        whole = R.maf_sample_bwd(x, pr["p"][:, :n], Ms, wz1, wl1, D, L, U, folded=True)
        tiled = R.maf_sample_bwd(x, pr["p"][:, :n], Ms, wz1, wl1, D, L, U, folded=True, tile=16)
        assert tiled[0].shape == whole[0].shape and x.shape[1] == 35  # two full tiles and three rows
        torch.testing.assert_close(tiled[0], whole[0], **TOL64)
        torch.testing.assert_close(tiled[1], whole[1], **TOL64)


# ---- the host half of tests/test_gpu_arsample_domain.py ------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(oracle):
    s = R.Sweep(tnf, oracle)
    for section in R.SECTIONS:
        s.need(section)
    return s


def test_sweep_grid_reaches_every_cell():
    """The counts are asserted so that a later edit of MR's grids cannot empty a cell silently."""
    domain = [(D, L, U) for D in range(2, 33) for L in (1, 2, 3) for U in range(5, 65)]
    shapes, refused = R.maf_shapes(), R.refused_shapes()
    assert len(MR.backward_cases()) == 48 and len(shapes) == 40 and len(refused) == 8
    assert {R.cell(*s) for s in shapes} == {R.cell(*s) for s in domain if MR.bwd_supported(*s)} and len({R.cell(*s) for s in shapes}) == 40
    assert sum(MR.nacc(*s) == 1 for s in shapes) == 12
    for s in MR.backward_cases():  # the refused shapes are exactly the library's
        assert (lib.tnf_maf_sample_bwd_supported(*s) == 0) == (s in refused), s
    # what tests/test_gpu_arsample.py's seven shapes never reach
    cells = {R.cell(*s) for s in shapes}
    assert {c for c in cells if c[1] == 4} and {c for c in cells if c[:2] == (1, 3)} and {c for c in cells if c[:2] == (2, 2)}
    assert {c for c in cells if c[0] == 2 and not c[2] and c[1] <= 2} and {c for c in cells if c[3] == 3 and c[1] > 1}
    assert any(s[0] == 17 for s in shapes)
    flow = R.flow_shapes()
    assert len(MR.train_cases()) == 24 and len(flow) == 20
    assert all(lib.tnf_maf_sample_bwd_supported(*s) == 1 and lib.tnf_ar_flow_supported(*s) == 1 for s in flow)
    assert {MR.tiles(s[0], s[2]) for s in R.nf_shapes()} == {MR.tiles(s[0], s[2]) for s in flow} and len(R.nf_shapes()) == 8
    assert [(MR.nacc(*s), R.vec(s[0])) for s in R.ARG_CELLS] == [(4, True), (4, False), (1, True), (1, False)]
    assert all(s in shapes for s in R.ARG_CELLS) and R.ALIGN_CELL[0] == 16 and MR.nacc(*R.ALIGN_CELL) == 4
    assert [MR.nacc(*s) for s in MR.LONG_CELLS] == [1, 4] and all(MR.bwd_supported(*s) for s in MR.LONG_CELLS)
    assert MR.bwd_bx(MR.LONG_N, 1) == 512 and MR.tiles_per_wave(MR.LONG_N, 512) == 2
    assert MR.bwd_supported(*MR.SMALL_WEIGHT[:3])
    with pytest.raises(Exception):  # D = 1: supported by the predicate, but the package builds no masks for it
        tnf.MAF(1, 1, 5)
    assert lib.tnf_maf_sample_bwd_supported(1, 1, 5) == 1


def test_sweep_noise_table(sweep):
    """The float32 folded restatement against the float64 restatement per group (quantity, L) on the sweep's own inputs:
    above rounding to nothing, and 4 x it within CAP for every group but the small-weight one."""
    print("\n" + sweep.table())
    assert (len(sweep.maf), len(sweep.args), len(sweep.flow), len(sweep.nf)) == (40 * 3, 4 * 6, 20 * 2, 8)
    for (name, L), v in sorted(sweep.noise.items()):
        assert 1e-9 < v and (name.startswith("small-weight") or sweep.bar(name, L) <= R.CAP), (name, L, v)


def test_planted_defects_fail_the_bars(sweep):
    """One sweep too few at D = 2, the - g_ld term dropped from d_alpha, GS left out of g_a: each in float64 on the
    smallest cell where it shows, each at least 10 x outside its group's bar."""
    s = (2, 1, 5)
    c = sweep.maf[(s, MR.BWD_ROWS[0])]
    args = (c.x.double(), c.params.double(), c.Ms, c.g_x.double(), c.g_ld.double(), *s)
    for defect in (dict(sweeps=0), dict(drop_gld=True)):
        got = R.maf_sample_bwd(*args, **defect)
        ratios = [MR.gerr(got[i], c.f64[i]) / sweep.bar("maf " + part, 1) for i, part in enumerate(("g_omega", "g_params"))]
        print("planted %s: %.1f, %.1f x the bar" % (defect, *ratios))
        assert max(ratios) >= 10.0
    s = R.flow_shapes()[0]
    f = sweep.flow[(s, R.FLOW_ROWS[0])]
    got = R.ar_flow_sample_bwd(f.z.double(), f.params.double(), f.Ms, *(t.double() for t in f.stat), f.g_z.double(),
                               f.g_sld.double(), *s, drop_gs=True)
    ratio = MR.gerr(f.split(got)[1], f.split(f.f64["both"])[1]) / sweep.bar("flow g_affine", s[1])
    print("planted GS left out of g_a: %.1f x the bar" % ratio)
    assert ratio >= 10.0 and MR.gerr(f.split(got)[0], f.split(f.f64["both"])[0]) == 0.0


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared():
    text = open(os.path.join(ROOT, "include", "tnf_arsample.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip() and p.strip() != "void"] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.ARSAMPLE_SIGNATURES) == sorted(NAMES) and len(protos) == 5
    others = set()
    for table in ("SIGNATURES", "MOG_SIGNATURES", "ABC_SIGNATURES", "HEBB_SIGNATURES", "EFN_SIGNATURES",
                  "PADTRAIN_SIGNATURES", "PADBATCH_SIGNATURES", "CTXFLOW_SIGNATURES", "CTXTRAIN_SIGNATURES",
                  "SAMPLETRAIN_SIGNATURES"):
        others |= set(getattr(_lib, table))
    assert not set(_lib.ARSAMPLE_SIGNATURES) & others  # disjoint from the other ten
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.ARSAMPLE_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    assert _lib.ARSAMPLE_SIGNATURES["tnf_arsample_launch_count"][0] is ctypes.c_int64
    assert _lib.ARSAMPLE_SIGNATURES["tnf_ar_flow_sample_bwd_workspace_bytes"][0] is ctypes.c_int64
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_arsample.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+\s*\(", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    assert _lib.DIAG_FAMILIES == 19  # a counter of its own: the flow families are a closed set
    assert lib.tnf_arsample_launch_count() >= 0


def _maf_bwd_mfma_supported(D, L, U):
    """maf_bwd_mfma_supported (csrc/maf_bwd_mfma.hip, no export of its own) restated: D <= 32, L <= 3, U <= 64, and both
    operand images, one accumulator copy, the transpose scratch and the constants within 156 KB of LDS."""
    if not (1 <= D <= 32 and 1 <= L <= 3 and 1 <= U <= 64):
        return False
    UT, DT = (U + 15) // 16, (D + 15) // 16
    nwg = 4 * UT * DT + (L - 1) * 2 * UT * UT
    floats = nwg * 256 + ((L - 1) * 2 * UT + 2 * DT) * 16 + 2 * nwg * 256 + 4 * 2 * 272 + 11 * 16 * DT + 4
    return floats * 4 <= 156 * 1024


def test_supported_is_the_domain_of_the_matrix_pipe_maf_backward():
    ones = 0
    for D in list(range(1, 35)) + [48, 64]:
        for L in range(1, 5):
            for U in (1, 15, 16, 17, 32, 42, 48, 49, 64, 65):
                got = lib.tnf_maf_sample_bwd_supported(D, L, U)
                assert got == int(_maf_bwd_mfma_supported(D, L, U)), (D, L, U)
                # tnf_ar_flow_train_supported is that predicate AND the forward kernel's
                assert (lib.tnf_ar_flow_train_supported(D, L, U) == 1) == (got == 1 and lib.tnf_ar_flow_supported(D, L, U) == 1)
                assert arsample_ops.maf_sample_bwd_supported(D, L, U) == bool(got)
                ones += got
    assert ones > 300  # not vacuous
    assert lib.tnf_maf_sample_bwd_supported(33, 2, 15) == 0 and lib.tnf_maf_sample_bwd_supported(6, 4, 15) == 0
    assert lib.tnf_maf_sample_bwd_supported(32, 3, 16) == 1 and lib.tnf_maf_sample_bwd_supported(21, 2, 42) == 1
    assert lib.tnf_maf_sample_bwd_supported(0, 2, 15) == 0 and lib.tnf_maf_sample_bwd_supported(6, 2, 0) == 0


def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(10)]  # never dereferenced: every call fails validation first
    count = arsample_ops.arsample_launch_count()
    diag = [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]
    D, L, U = 6, 2, 15
    Pm = lib.tnf_maf_num_params(D, L, U)
    big = 1 << 40

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    def maf(**kw):
        a = dict(x=p[0], params=p[1], masks=p[2], g_x=p[3], g_ld=p[4], g_omega=p[5], g_params=p[6], M=3, Mp=3, N=40, D=D,
                 L=L, U=U, pstride=Pm, gpstride=Pm)
        a.update(kw)
        return lib.tnf_maf_sample_bwd_f32(a["x"], a["params"], a["masks"], a["g_x"], a["g_ld"], a["g_omega"], a["g_params"],
                                          a["M"], a["Mp"], a["N"], a["D"], a["L"], a["U"], a["pstride"], a["gpstride"], None)

    def flow(**kw):
        a = dict(z=p[0], params=p[1], masks=p[2], mean=p[3], alpha=p[4], g_z=p[5], g_sld=p[6], g_params=p[7], M=3, Mp=3,
                 N=40, D=D, L=L, U=U, pstride=Pm + 2 * D, gpstride=Pm + 2 * D, ws=p[8], ws_bytes=big)
        a.update(kw)
        return lib.tnf_ar_flow_sample_bwd_f32(a["z"], a["params"], a["masks"], a["mean"], a["alpha"], a["g_z"], a["g_sld"],
                                              a["g_params"], a["M"], a["Mp"], a["N"], a["D"], a["L"], a["U"], a["pstride"],
                                              a["gpstride"], a["ws"], a["ws_bytes"], None)

    for call, tag, ptrs, both, need in (
            (maf, b"tnf_maf_sample_bwd_f32", ("x", "params", "masks", "g_params"), dict(g_x=None, g_ld=None), Pm),
            (flow, b"tnf_ar_flow_sample_bwd_f32", ("z", "params", "masks", "mean", "alpha", "g_params"),
             dict(g_z=None, g_sld=None), Pm + 2 * D)):
        for name in ptrs:
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        refused(call(**both), INV, tag + b": g_")
        for kw in (dict(M=0), dict(M=-3), dict(Mp=2), dict(Mp=0), dict(N=-1), dict(M=1, Mp=3)):
            refused(call(**kw), INV, tag + b": M=")
        for kw in (dict(D=33), dict(D=0), dict(L=4), dict(L=0), dict(U=65), dict(U=0)):
            refused(call(**kw), UNSUP, tag + b": no kernel for D=")
        refused(call(pstride=need - 1), INV, tag + b": parameter rows shorter than %d" % need)
        refused(call(gpstride=need - 1), INV, tag + b": parameter rows shorter than %d" % need)
        refused(call(g_params=p[1]), INV, tag + b": g_params must not alias params")
        assert call(N=0) == 0  # nothing to do: OK, no launch
        refused(call(N=0, gpstride=need - 1), INV, tag + b": parameter rows shorter")  # ... after the other checks
    assert maf(g_omega=None, N=0) == 0 and maf(g_x=None, N=0) == 0 and flow(g_sld=None, N=0) == 0
    q = lib.tnf_ar_flow_sample_bwd_workspace_bytes
    need = q(3, D)
    assert need >= 4 * (3 * 2 * D + 3 * (2 * D + 1)) and need % 16 == 0 and q(1, D) < need
    assert q(0, D) == INV and q(3, 0) == INV
    for kw in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert flow(**kw) == WS and b"tnf_ar_flow_sample_bwd_f32" in lib.tnf_last_error()
    assert flow(ws_bytes=need, N=0) == 0
    assert arsample_ops.arsample_launch_count() == count  # nothing was launched
    assert [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)] == diag


# ---- routing -------------------------------------------------------------------------------------------------------------
TRAIN = "ar_flow_sample_train"


def run_row(r, switch):
    """test_route_table.run_row with `NormFlow.ar_sample_training` = switch and the new module's entry recorded."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(tnf.NormFlow, "ar_sample_training", switch)
        trace = []

        def recorder(*args, **kwargs):
            trace.append(TRAIN)
            raise RT._Reached()

        mp.setattr(arsample_ops, TRAIN, recorder)
        out = RT.run_row(r)
    return out + trace


def test_switch_off_is_todays_route_on_the_ar_rows_of_the_grid():
    table, seen, changed = RT._table(), 0, 0
    for r in RT.GRID:
        if r["arch"] != "AR":
            continue
        old = table[RT.row_id(r)]
        assert run_row(r, False) == old, RT.row_id(r)
        seen += 1
        candidate = r["op"] == "forward" and r["freeze_bn"] and r["p_grad"] and not r["no_grad"]
        if candidate:  # switch on: only these may change hands, and only from the per-bijector composition
            on = run_row(r, True)
            if on != old:
                assert on[-1] == TRAIN and "maf" in old and not r["stats_graph"], RT.row_id(r)
                changed += 1
    assert seen > 0


def test_family_and_its_exclusions():
    assert tnf.NormFlow.ar_sample_training is False and tnf.MAF.fused_sampling_backward is False
    nf = tnf.NormFlow(6, True, "AR", 1, 2, 15, device="cpu")
    om, p = torch.zeros(3, 40, 6), torch.zeros(3, nf.D_params, requires_grad=True)
    today = nf._route("forward", om, p)
    assert today.family == "bijectors"  # the switch defaults to off
    nf.ar_sample_training = True
    assert nf._route("forward", om, p) == ("ar_train_sample", False, False)
    assert nf._route("forward", om, p, f32_draw=True) == ("ar_train_sample", False, False)
    assert nf._route("forward", om, p[:1]).family == "ar_train_sample"  # one shared row
    assert nf._route("forward", om[:, :1], p).family == "ar_train_sample"  # per-context rows: any N >= 1
    assert nf._route("forward", om, p, freeze_bn=False).family == "bijectors"  # fresh statistics: the composition
    assert nf._route("forward", om, p.detach()).family == "ar_fused"  # params without grad: the inference kernel
    with torch.no_grad():
        assert nf._route("forward", om, p).family == "ar_fused"
    assert nf._route("log_prob", om, p).family == "ar_train" and nf._route("inverse", om, p).family != "ar_train_sample"
    assert nf._route("forward", om.double(), p.double()).family == "bijectors"  # float64
    assert nf._route("forward", om[0], p).family == "bijectors"  # 2-d
    assert nf._route("forward", om[:1], p).family == "bijectors"  # M_z = 1 < M_p
    assert nf._route("forward", om, torch.zeros(2, nf.D_params, requires_grad=True)).family == "bijectors"  # M_p not in {1, M}
    from torch_nf_amd import ops
    with pytest.MonkeyPatch.context() as mp:  # the bf16 operand experiment keeps today's route
        mp.setattr(ops, "current_operand_precision", lambda: "bf16")
        assert nf._route("forward", om, p).family == "bijectors"
    nf.bijectors[1]._last_mean = torch.zeros(6, requires_grad=True)  # statistics carrying a graph
    assert nf._route("forward", om, p).family == "bijectors"
    wide = tnf.NormFlow(33, True, "AR", 1, 2, 15, device="cpu")  # D = 33
    wide.ar_sample_training = True
    assert wide._route("forward", torch.zeros(1, 8, 33), torch.zeros(1, wide.D_params, requires_grad=True)).family == "bijectors"
    for support in (tnf.ToInterval(6, [-1.0] * 6, [2.0] * 6), tnf.ToSimplex(6)):  # any support layer: its own op behind
        sup = tnf.NormFlow(6, True, "AR", 1, 2, 15, support, device="cpu")
        ps = torch.zeros(1, sup.D_params, requires_grad=True)
        off = sup._route("forward", torch.zeros(1, 8, 6), ps)
        sup.ar_sample_training = True
        assert off.family == "bijectors" and sup._route("forward", torch.zeros(1, 8, 6), ps) == ("ar_train_sample", False, False)
    cp = tnf.NormFlow(6, True, "coupling", 2, 2, 15, device="cpu")
    cp.ar_sample_training = True
    assert cp._route("forward", om, torch.zeros(3, cp.D_params, requires_grad=True)).family != "ar_train_sample"


def test_maf_switch_is_decided_in_forward():
    """ops.maf passes the switch to the autograd node; where the fused call does not apply the node keeps today's code."""
    from torch_nf_amd import ops

    x32, p32 = torch.zeros(2, 5, 6), torch.zeros(2, 4)
    assert arsample_ops.maf_sample_route_ok(x32, p32, 6, 2, 15) and arsample_ops.maf_sample_route_ok(x32, p32[:1], 6, 2, 15)
    assert not arsample_ops.maf_sample_route_ok(x32.double(), p32.double(), 6, 2, 15)
    assert not arsample_ops.maf_sample_route_ok(torch.zeros(2, 5, 33), p32, 33, 2, 15)
    assert not arsample_ops.maf_sample_route_ok(x32, torch.zeros(3, 4), 6, 2, 15)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "current_operand_precision", lambda: "bf16")
        assert not arsample_ops.maf_sample_route_ok(x32, p32, 6, 2, 15)
    assert ops.maf.__defaults__ == (False,)
