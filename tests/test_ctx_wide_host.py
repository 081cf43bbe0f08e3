"""The wide per-context kernels (include/tnf_ctxwide.h, csrc/flow_ctx_wide.hip, csrc/flow_ctx_wide_bwd.hip, NormFlow's
families `context_rows_wide` and `train_context_wide`), without a GPU: header, exports and binding table in step; both
support predicates and the LDS query against their restated definitions over the whole domain; the existing predicates
unchanged; every refusal that precedes a launch; the restated arithmetic against the oracle in float64, values and
gradients, with planted defects that must fail; and the routing of NormFlow with the switches on and off."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT, grad_err
import ctxwide_restatement as R
import test_gpu_ctx_flow as CF
import wideflow_restatement as W
from domain_helpers import BAR_P, BAR_Z, float64

import torch_nf_amd as tnf
from torch_nf_amd import _lib, ctxflow_ops, ctxtrain_ops, ctxwide_ops, wideflow_ops

lib = _lib.lib
INV, UNSUP = -1, -2  # TNF_EINVAL, TNF_EUNSUPPORTED
HEADER = os.path.join(ROOT, "include", "tnf_ctxwide.h")
NAMES = ("tnf_ctx_wide_supported", "tnf_ctx_wide_train_supported", "tnf_ctx_wide_lds_bytes", "tnf_ctx_wide_launch_count",
         "tnf_ctx_wide_log_prob_f32", "tnf_ctx_wide_forward_f32", "tnf_ctx_wide_log_prob_bwd_f32")
OTHER_TABLES = ("SIGNATURES", "MOG_SIGNATURES", "ABC_SIGNATURES", "HEBB_SIGNATURES", "EFN_SIGNATURES", "PADTRAIN_SIGNATURES",
                "PADBATCH_SIGNATURES", "CTXFLOW_SIGNATURES", "CTXTRAIN_SIGNATURES", "SAMPLETRAIN_SIGNATURES",
                "ARSAMPLE_SIGNATURES", "ARBATCH_SIGNATURES", "CTXSAMPLE_SIGNATURES", "WIDEFLOW_SIGNATURES")


# ---- the C ABI, host side ------------------------------------------------------------------------------------------------
def _declared(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    return {name: [p for p in params.split(",") if p.strip()] for name, params in protos}


def test_header_exports_and_bindings_in_step():
    protos = _declared()
    assert sorted(protos) == sorted(_lib.CTXWIDE_SIGNATURES) == sorted(NAMES)
    tables = [n for n in dir(_lib) if n.endswith("SIGNATURES") and n != "CTXWIDE_SIGNATURES"]
    assert set(OTHER_TABLES) == set(tables)  # a fifteenth table
    for n in tables:
        assert not set(_lib.CTXWIDE_SIGNATURES) & set(getattr(_lib, n)), n
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, params in protos.items():
        assert hasattr(raw, name), "libtnf_hip.so does not export %s" % name
        res, args = _lib.CTXWIDE_SIGNATURES[name]
        assert len(args) == len(params), name
        for p, a in zip(params, args):  # void*, int64_t and int32_t
            want = ctypes.c_void_p if "*" in p else ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert a is want and ("*" in p or "int64_t" in p or "int32_t" in p), (name, p)
        assert getattr(_lib.lib, name).argtypes == args
    for name in ("tnf_ctx_wide_launch_count", "tnf_ctx_wide_lds_bytes"):
        assert _lib.CTXWIDE_SIGNATURES[name][0] is ctypes.c_int64
    # the arguments are exactly those of the 16-unit entries
    for new, old, table in (("tnf_ctx_wide_log_prob_f32", "tnf_ctx_flow_log_prob_f32", _lib.CTXFLOW_SIGNATURES),
                            ("tnf_ctx_wide_forward_f32", "tnf_ctx_flow_forward_f32", _lib.CTXFLOW_SIGNATURES),
                            ("tnf_ctx_wide_log_prob_bwd_f32", "tnf_ctx_train_log_prob_bwd_f32", _lib.CTXTRAIN_SIGNATURES),
                            ("tnf_ctx_wide_supported", "tnf_ctx_flow_supported", _lib.CTXFLOW_SIGNATURES),
                            ("tnf_ctx_wide_train_supported", "tnf_ctx_train_supported", _lib.CTXTRAIN_SIGNATURES)):
        assert _lib.CTXWIDE_SIGNATURES[new] == table[old]
        header_old = os.path.join(ROOT, "include", "tnf_ctxflow.h" if table is _lib.CTXFLOW_SIGNATURES else "tnf_ctxtrain.h")
        assert [re.sub(r"\s+", " ", p).strip() for p in protos[new]] == \
            [re.sub(r"\s+", " ", p).strip() for p in _declared(header_old)[old]]
    header = open(HEADER).read()
    tnf_h = open(os.path.join(ROOT, "include", "tnf.h")).read()
    assert '#include "tnf_ctxwide.h"' in tnf_h and not set(protos) & set(re.findall(r"\btnf_[a-z0-9_]+", re.sub(
        r"/\*.*?\*/", "", tnf_h, flags=re.S)))  # tnf.h points to the header and declares none of its entries
    for i, n in enumerate(("LOG_PROB", "FORWARD", "LOG_PROB_BWD")):
        assert "TNF_CTXWIDE_COUNT_%s = %d" % (n, i) in header
    assert "TNF_CTXWIDE_COUNTERS = 3" in header
    assert (ctxwide_ops.COUNT_LOG_PROB, ctxwide_ops.COUNT_FORWARD, ctxwide_ops.COUNT_LOG_PROB_BWD) == (0, 1, 2)
    assert _lib.DIAG_FAMILIES == 19  # a counter space of its own: the flow families are a closed set
    for which in range(3):
        assert lib.tnf_ctx_wide_launch_count(which) >= 0
    assert lib.tnf_ctx_wide_launch_count(3) == -1 and b"tnf_ctx_wide_launch_count" in lib.tnf_last_error()
    assert lib.tnf_ctx_wide_launch_count(-1) == -1
    makefile = open(os.path.join(ROOT, "torch_nf_amd", "csrc", "Makefile")).read()
    for word in ("flow_ctx_wide.hip", "flow_ctx_wide_bwd.hip", "ctx_wide.h", "../../include/tnf_ctxwide.h"):
        assert word in makefile, word


def test_predicates_and_lds_are_their_definitions_over_the_domain():
    """D 1 .. 65, L 0 .. 6, U 15 .. 65, N in {0, 1, 16, 31, 32}, S in {0, 1, 9}: both predicates, both LDS queries and the
    ops wrappers against the restated definitions; the shapes every design must accept are accepted."""
    ones = [0, 0]
    for D in range(1, 66):
        for L in range(0, 7):
            for U in range(15, 66):
                for N in (0, 1, 16, 31, 32):
                    for S in (0, 1, 9):
                        a = (D, S, L, U, N)
                        fwd, trn = R.ctx_wide_supported(*a), R.ctx_wide_train_supported(*a)
                        assert lib.tnf_ctx_wide_supported(*a) == int(fwd), a
                        assert lib.tnf_ctx_wide_train_supported(*a) == int(trn), a
                        for which in (R.FWD, R.BWD) + ((2, -1) if U % 16 == 1 else ()):
                            assert lib.tnf_ctx_wide_lds_bytes(which, *a) == R.lds_bytes(which, *a), (which, a)
                        ones[0] += fwd
                        ones[1] += trn
                        if R.in_domain(D, S, U, N) and (1 <= L <= 2 or (L == 3 and U <= 48)):
                            assert fwd and trn, a  # guaranteed whatever the design
                        if not (2 <= D <= 64 and S >= 1 and 17 <= U <= 64 and 1 <= N <= 31):
                            assert not fwd and not trn
    assert ones[0] > 80000 and ones[1] > 40000, ones
    assert ctxwide_ops.ctx_wide_supported(5, 2, 2, 20, 8) and ctxwide_ops.ctx_wide_train_supported(5, 2, 2, 20, 8)
    assert not ctxwide_ops.ctx_wide_supported(5, 2, 2, 16, 8) and not ctxwide_ops.ctx_wide_train_supported(5, 2, 2, 20, 32)
    assert ctxwide_ops.lds_bytes(ctxwide_ops.LDS_FORWARD, 5, 2, 2, 20, 8) == R.lds_bytes(R.FWD, 5, 2, 2, 20, 8)
    # the sizes worked out for the design
    assert R.lds_bytes(R.FWD, 32, 1, 5, 64, 1) == 150400 and R.ctx_wide_supported(32, 1, 5, 64, 31)
    assert R.lds_bytes(R.FWD, 33, 1, 5, 49, 1) == 167168 and not R.ctx_wide_supported(33, 1, 5, 49, 1)
    assert R.ctx_wide_supported(64, 1, 5, 48, 31) and R.ctx_wide_supported(64, 1, 4, 64, 31)
    assert R.lds_bytes(R.BWD, 64, 1, 2, 64, 31) == 123008
    assert R.lds_bytes(R.BWD, 33, 1, 3, 64, 31) == 144512 and R.ctx_wide_train_supported(33, 1, 3, 64, 31)
    assert R.lds_bytes(R.BWD, 64, 1, 3, 64, 31) == 172160 and not R.ctx_wide_train_supported(64, 1, 3, 64, 31)
    assert R.lds_bytes(R.BWD, 64, 1, 3, 64, 1) == 102928 and R.ctx_wide_train_supported(64, 1, 3, 64, 1)
    assert max(N for N in range(1, 32) if R.ctx_wide_train_supported(64, 1, 3, 64, N)) == TOP_N_D64_L3_U64
    # S is unbounded and independent of the LDS; the sample count is a 64-bit argument
    assert lib.tnf_ctx_wide_supported(64, 1 << 30, 4, 64, 31) == 1 and lib.tnf_ctx_wide_train_supported(64, 1 << 30, 2, 64, 31) == 1
    assert lib.tnf_ctx_wide_supported(5, 2, 2, 20, 1 << 40) == 0 and lib.tnf_ctx_wide_train_supported(5, 2, 2, 20, -1) == 0
    assert lib.tnf_ctx_wide_lds_bytes(0, 5, 2, 1 << 20, 20, 1) == 4 * W.layer_floats(5, 1 << 20, 20)  # any L >= 1: a size


TOP_N_D64_L3_U64 = 22  # the header's example


def test_existing_predicates_keep_their_values():
    for D in (1, 2, 5, 32, 33, 64, 65):
        for L in (0, 1, 3, 4, 5, 6):
            for U in (15, 16, 17, 64, 65):
                for N in (0, 1, 31, 32):
                    for S in (0, 1, 9):
                        narrow = 2 <= D <= 64 and S >= 1 and 1 <= L <= 3 and 1 <= U <= 16 and 1 <= N <= 31
                        assert lib.tnf_ctx_flow_supported(D, S, L, U, N) == int(narrow)
                        assert lib.tnf_ctx_train_supported(D, S, L, U, N) == int(narrow)
                        assert lib.tnf_wide_flow_supported(D, S, L, U) == int(W.wide_flow_supported(D, S, L, U))
                        # the unit ranges are disjoint: nothing changes hands
                        assert not (narrow and (lib.tnf_ctx_wide_supported(D, S, L, U, N) or
                                                lib.tnf_ctx_wide_train_supported(D, S, L, U, N)))
    assert lib.tnf_wide_flow_supported(5, 1, 2, 16) == 0 and lib.tnf_wide_flow_supported(5, 1, 2, 17) == 1
    assert lib.tnf_ctx_flow_supported(5, 1, 2, 16, 8) == 1 and lib.tnf_ctx_flow_supported(5, 1, 2, 17, 8) == 0
    assert lib.tnf_ctx_train_supported(5, 1, 2, 16, 8) == 1 and lib.tnf_ctx_train_supported(5, 1, 2, 17, 8) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------
def _others():
    return (ctxflow_ops.launch_counts(), ctxtrain_ops.launch_count(), wideflow_ops.launch_counts(),
            [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)])


def test_argument_refusals_without_launching():
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]  # never dereferenced: every call fails validation first
    counts, others = ctxwide_ops.launch_counts(), _others()

    def refused(rc, code, text):
        msg = lib.tnf_last_error()
        assert rc == code and text in msg, (rc, code, msg)

    P5 = lib.tnf_flow_num_params(5, 2, 2, 20)
    assert P5 == R.flow_params(5, 2, 2, 20)

    def log_prob(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], lp=p[4], z0=p[5], sld=p[6], Mz=3, M=3, N=8, D=5, S=2, L=2, U=20,
                 pstride=P5)
        a.update(kw)
        return lib.tnf_ctx_wide_log_prob_f32(a["z"], a["params"], a["mean"], a["alpha"], a["lp"], a["z0"], a["sld"], a["Mz"],
                                             a["M"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    def forward(**kw):
        a = dict(z=p[0], params=p[1], mean=p[2], alpha=p[3], z0=p[5], sld=p[6], M=3, N=8, D=5, S=2, L=2, U=20, pstride=P5)
        a.update(kw)
        return lib.tnf_ctx_wide_forward_f32(a["z"], a["params"], a["mean"], a["alpha"], a["z0"], a["sld"], a["M"], a["N"],
                                            a["D"], a["S"], a["L"], a["U"], a["pstride"], None)

    def bwd(**kw):
        a = dict(z0=p[0], params=p[1], mean=p[2], alpha=p[3], g_lp=p[4], g_params=p[5], g_z=p[6], M=3, N=8, D=5, S=2, L=2,
                 U=20, pstride=P5, gpstride=P5)
        a.update(kw)
        return lib.tnf_ctx_wide_log_prob_bwd_f32(a["z0"], a["params"], a["mean"], a["alpha"], a["g_lp"], a["g_params"],
                                                 a["g_z"], a["M"], a["N"], a["D"], a["S"], a["L"], a["U"], a["pstride"],
                                                 a["gpstride"], None)

    shapes = (dict(D=1), dict(D=65), dict(D=0), dict(L=0), dict(U=16), dict(U=15), dict(U=65), dict(U=0), dict(S=0),
              dict(N=32), dict(N=1000))
    for call, tag in ((log_prob, b"tnf_ctx_wide_log_prob_f32"), (forward, b"tnf_ctx_wide_forward_f32")):
        for name in ("z", "params", "mean", "alpha"):
            refused(call(**{name: None}), INV, tag + b": NULL pointer")
        for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
            refused(call(**kw), INV, tag + b": M_z=")
        for kw in shapes + (dict(L=6), dict(D=33, L=5, U=49)):
            refused(call(**kw), UNSUP, tag + b": no wide per-context kernel for D=")
        refused(call(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
        assert call(N=0) == 0  # nothing to do: OK, no launch
        refused(call(N=0, pstride=P5 - 1), INV, tag + b": params row has")  # ... after the other checks
    for kw in (dict(Mz=2), dict(Mz=0), dict(Mz=4)):
        refused(log_prob(**kw), INV, b"tnf_ctx_wide_log_prob_f32: M_z=")
    refused(log_prob(lp=None, z0=None, sld=None), INV, b"tnf_ctx_wide_log_prob_f32: no output requested")
    refused(forward(z0=None, sld=None), INV, b"tnf_ctx_wide_forward_f32: no output requested")
    refused(log_prob(z0=p[0]), INV, b"z0 must not alias z")
    refused(forward(z0=p[0]), INV, b"z_out must not alias omega")
    assert log_prob(Mz=1, N=0) == 0 and log_prob(lp=None, sld=None, N=0) == 0 and forward(sld=None, N=0) == 0

    tag = b"tnf_ctx_wide_log_prob_bwd_f32"
    for name in ("z0", "params", "mean", "alpha", "g_lp", "g_params"):
        refused(bwd(**{name: None}), INV, tag + b": NULL pointer")
    for kw in (dict(M=0), dict(M=-3), dict(N=-1)):
        refused(bwd(**kw), INV, tag + b": M=")
    for kw in shapes + (dict(L=4), dict(D=64, L=3, U=64, N=31)):
        refused(bwd(**kw), UNSUP, tag + b": no wide per-context backward for D=")
    refused(bwd(pstride=P5 - 1), INV, tag + b": params row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(gpstride=P5 - 1), INV, tag + b": gradient row has %d elements, flow needs %d" % (P5 - 1, P5))
    refused(bwd(pstride=0), INV, tag + b": params row has 0 elements")
    refused(bwd(g_z=p[0]), INV, tag + b": g_z must not alias z0")
    refused(bwd(g_params=p[1]), INV, tag + b": g_params must not alias params")
    assert bwd(N=0) == 0 and bwd(N=0, g_z=None) == 0  # nothing to do: OK, no launch
    refused(bwd(N=0, gpstride=P5 - 1), INV, tag + b": gradient row has")  # ... after the other checks
    assert ctxwide_ops.launch_counts() == counts and _others() == others  # nothing was launched


# ---- the restatement ---------------------------------------------------------------------------------------------------
RESTATED = [(2, 1, 2, 20, 3, 1), (3, 2, 2, 17, 3, 15), (4, 1, 2, 20, 5, 1), (5, 2, 3, 33, 3, 17), (8, 1, 1, 64, 3, 16),
            (31, 1, 2, 48, 3, 31), (33, 2, 2, 20, 3, 7), (64, 1, 2, 64, 2, 31), (5, 9, 2, 20, 2, 4)]


def _case(oracle, D, S, L, U, M, N):
    params, mean, alpha, z = CF.inputs(oracle, D, S, L, U, M, N)
    return params, (mean, alpha), z


@pytest.mark.parametrize("case", RESTATED, ids=R.case_id)
def test_restatement_is_the_oracle_in_float64(oracle, case):
    """Even and odd D, D = 2 and 3, one and two tiles, both directions, one block of z per context and one for all, values
    and -- by autograd through the restatement and through the oracle -- gradients: 1e-12.  Padded slots are exactly 0."""
    D, S, L, U, M, N = case
    shape = (D, S, L, U)
    params, stat, z = _case(oracle, *case)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(7)).double()
    with float64():
        st64 = CF.st64(*stat)
        stat64 = (stat[0].double(), stat[1].double())
        for zz in (z, z[:1]):
            ze = zz.double().expand(M, N, D).contiguous()
            p_o, z_o = params.double().requires_grad_(), ze.clone().requires_grad_()
            z0_w, sld_w = oracle.flow_inverse(z_o, p_o, *shape, st64)
            lp_w = oracle.flow_log_prob(z_o, p_o, *shape, st64)
            (lp_w * g).sum().backward()
            p_r, z_r = params.double().requires_grad_(), zz.double().clone().requires_grad_()
            lp, z0, sld = R.ctx_wide_log_prob(z_r, p_r, *shape, stat64)
            (lp * g).sum().backward()
            for k, got, want in (("lp", lp, lp_w), ("z0", z0, z0_w), ("sld", sld, sld_w)):
                assert got.dtype == torch.float64 and got.shape == want.shape
                assert W.err(got, want) <= 1e-12, k
            gz_w = z_o.grad if zz.shape[0] == M else z_o.grad.sum(0, keepdim=True)  # a shared block: summed over contexts
            assert grad_err("ctxwide restatement f64 params", p_r.grad, p_o.grad) <= 1e-12
            assert grad_err("ctxwide restatement f64 z", z_r.grad, gz_w) <= 1e-12
        with torch.no_grad():
            zf, sldf, pad = R.ctx_wide_forward(z.double(), params.double(), *shape, stat64)
            zf_w, lq_w, _ = oracle.flow_forward(z.double().numpy(), params.double(), *shape, st64)
            sldf_w = torch.from_numpy(oracle.base_log_density_f64(z.double().numpy())) - lq_w
            assert pad == 0.0  # the padding stays exactly 0 through every layer
            assert W.err(zf, zf_w) <= 1e-12 and W.err(sldf, sldf_w) <= 1e-12
            back = R.ctx_wide_log_prob(zf, params.double(), *shape, stat64)[1]
            assert W.err(back, z.double()) <= 1e-9  # the round trip
    with torch.no_grad():  # float32: the padding is exactly zero there too
        assert R.ctx_wide_forward(z, params, *shape, stat)[2] == 0.0


@pytest.mark.parametrize("defect", ["pad_weight", "pad_fold"])
@pytest.mark.parametrize("case", [(3, 2, 2, 17, 3, 15), (5, 2, 3, 33, 3, 17), (33, 2, 2, 20, 3, 7)], ids=R.case_id)
def test_planted_defects_fail(oracle, case, defect):
    """A non-zero operand in a padded slot of the image, or a padded slot of the fold that is not (1, 0), breaks the
    float64 agreement by many orders of magnitude: the check above can fail."""
    D, S, L, U, M, N = case
    params, stat, z = _case(oracle, *case)
    with float64(), torch.no_grad():
        stat64 = (stat[0].double(), stat[1].double())
        lp = R.ctx_wide_log_prob(z.double(), params.double(), D, S, L, U, stat64, defect=defect)[0]
        good = R.ctx_wide_log_prob(z.double(), params.double(), D, S, L, U, stat64)[0]
        want = oracle.flow_log_prob(z.double(), params.double(), D, S, L, U, CF.st64(*stat))
    assert W.err(good, want) <= 1e-12 < 1e-7 < W.err(lp, want)


def row_err(got, want):
    got, want = got.detach().double().flatten(1), want.detach().double().flatten(1)
    return float(((got - want).abs().max(1).values / want.abs().max(1).values.clamp_min(1e-300)).max())


@pytest.mark.parametrize("case", [(5, 2, 2, 20, 5, 8), (2, 1, 1, 17, 5, 1), (33, 2, 3, 48, 3, 17), (64, 1, 2, 64, 2, 31)],
                         ids=R.case_id)
def test_backward_walk_on_real_widths_against_float64_autograd(oracle, case):
    """The float32 walk from a float32 z0, explicit deltas on the real widths (no padded row, feature or unit), against
    float64 autograd through the oracle: within the bars of the GPU test, whole and per context row."""
    D, S, L, U, M, N = case
    params, stat, z = _case(oracle, *case)
    g = torch.randn(M, N, generator=torch.Generator().manual_seed(7))
    with float64():
        p64, z64 = params.double().requires_grad_(), z.double().requires_grad_()
        (oracle.flow_log_prob(z64, p64, D, S, L, U, CF.st64(*stat)) * g.double()).sum().backward()
    with torch.no_grad():
        z0 = R.ctx_wide_log_prob(z, params, D, S, L, U, stat)[1]  # the z0 the forward keeps
        gp, gz = R.ctx_wide_log_prob_bwd(z0, params, stat, g, D, S, L, U)
    assert gp.shape == params.shape and gz.shape == z.shape
    for name, got, want, bar in (("params", gp, p64.grad, BAR_P), ("z", gz, z64.grad, BAR_Z)):
        tag = "ctxwide restatement %s %s" % (name, R.case_id(case))
        print(tag, "whole %.2e per row %.2e" % (grad_err(tag, got, want), row_err(got, want)))
        grad_err(tag, got, want, bar)
        assert row_err(got, want) <= bar
    gpz, gzz = R.ctx_wide_log_prob_bwd(z0, params, stat, torch.zeros(M, N), D, S, L, U)
    assert not gpz.any() and not gzz.any()  # zero upstream gradient: exactly zero everywhere


def test_the_gpu_sweep_covers_its_cells():
    cases = R.forward_cases()
    assert 18 <= len(R.forward_shapes()) <= 24
    by_L = {L: sum(c[2] == L for c in cases) for L in (1, 2, 3, 5)}
    assert min(by_L.values()) >= 4, by_L  # no (quantity, L) group with fewer than four cases
    assert {c[5] for c in cases} == set(R.NS) and {c[4] for c in cases} == set(R.MS) and {1, 2, 9} <= {c[1] for c in cases}
    assert R.CDE_SHAPE + (5, 1) in cases
    assert {R.tiles(c[0], c[3]) + (c[2],) for c in cases} >= {(HT, UT, L) for HT in (1, 2) for UT in (2, 3, 4) for L in (1, 2, 3)}


# ---- routing -----------------------------------------------------------------------------------------------------------------
ROWS, TRAIN = ("context_rows_wide", False, False), ("train_context_wide", False, False)


def _flow(D, S, L, U, arch="coupling", **kw):
    nf = tnf.NormFlow(D, True, arch, S, L, U, device="cpu", **kw)
    return nf, torch.zeros(5, nf.D_params)


def test_switches_default_to_off_and_are_independent():
    assert tnf.NormFlow.wide_context_rows is False and tnf.NormFlow.wide_context_training is False
    nf, p = _flow(4, 1, 2, 20)
    assert "wide_context_rows" not in vars(nf) and "wide_context_training" not in vars(nf)
    z = torch.zeros(5, 8, 4)
    pg = p.clone().requires_grad_()
    with torch.no_grad():
        for op in ("log_prob", "inverse", "forward"):
            assert nf._route(op, z, p).family == "bijectors"  # U = 20, N = 8, M = 5: today's composition
    assert nf._route("log_prob", z, pg).family == "bijectors"
    for other in ("wide_flow", "context_rows", "context_training", "context_sample_training"):
        setattr(nf, other, True)  # no existing switch offers these calls to a one-launch family
    with torch.no_grad():
        for op in ("log_prob", "inverse", "forward"):
            assert nf._route(op, z, p).family == "bijectors"
    assert nf._route("log_prob", z, pg).family == "bijectors"
    nf.wide_context_rows = True
    with torch.no_grad():
        for op in ("log_prob", "inverse", "forward"):
            assert nf._route(op, z, p) == ROWS
    assert nf._route("log_prob", z, pg).family == "bijectors"  # the inference switch alone leaves autograd alone
    assert nf._route("log_prob", z, p) == ROWS  # grad mode on, nothing requires grad: plain
    nf.wide_context_rows, nf.wide_context_training = False, True
    assert nf._route("log_prob", z, pg) == TRAIN
    with torch.no_grad():
        assert nf._route("log_prob", z, pg).family == "bijectors"  # the training switch alone leaves inference alone
    assert nf._route("log_prob", z, p).family == "bijectors"  # nothing to train
    nf.wide_context_rows = True
    assert nf._route("log_prob", z, pg) == TRAIN and nf._route("log_prob", z, p) == ROWS


def test_families_and_their_exclusions():
    nf, p = _flow(5, 2, 2, 20)
    nf.wide_context_rows = nf.wide_context_training = True
    z, pg = torch.zeros(5, 8, 5), p.clone().requires_grad_()
    zg = torch.zeros(5, 8, 5, requires_grad=True)
    # training
    assert nf._route("log_prob", zg, p) == TRAIN and nf._route("log_prob", zg, pg) == TRAIN  # z alone, or both
    assert nf._route("log_prob", z[:1], pg) == TRAIN  # one shared block that needs no gradient
    assert nf._route("log_prob", zg[:1], pg).family == "bijectors"  # ... its gradient would sum over contexts
    assert nf._route("log_prob", torch.zeros(2, 8, 5), pg).family == "bijectors"  # M_z not in {1, M}
    assert nf._route("log_prob", z, pg[:1]).family not in (TRAIN[0], ROWS[0])  # one parameter row
    assert nf._route("inverse", z, pg).family == "bijectors" and nf._route("forward", z, pg).family == "bijectors"
    with torch.no_grad():
        assert nf._route("log_prob", z[:1], p) == ROWS and nf._route("inverse", z[:1], p) == ROWS
        assert nf._route("forward", z[:1], p).family == "bijectors"  # sampling: one block of draws per row
        assert nf._route("log_prob", z, p[:1]).family != ROWS[0]

    def unchanged(op, z, p, **kw):
        """With both switches on the call takes the route it takes with both off."""
        on = nf._route(op, z, p, **kw)
        nf.wide_context_rows = nf.wide_context_training = False
        off = nf._route(op, z, p, **kw)
        nf.wide_context_rows = nf.wide_context_training = True
        assert on == off and on.family not in (ROWS[0], TRAIN[0]), (op, on, off)

    for pp in (p, pg):
        unchanged("log_prob", torch.zeros(5, 32, 5), pp)  # N = 32
        unchanged("log_prob", z, pp[:1])  # one parameter row
        unchanged("log_prob", z.double(), pp)  # float64
        unchanged("log_prob", z, pp.double())
        unchanged("log_prob", z[0], pp)  # 2-d z
        unchanged("forward", z, pp, freeze_bn=False)  # fresh statistics
        nf.fusion = _lib.FUSE_LAYER
        unchanged("log_prob", z, pp)
        unchanged("forward", z, pp)
        nf.fusion = _lib.FUSE_FLOW
        assert nf._route("log_prob", z, pp) == (TRAIN if pp is pg else ROWS)
        nf.fusion = _lib.FUSE_AUTO
    bn = nf._bn_layers()[0]
    keep = bn._last_mean
    bn._last_mean = torch.zeros(5, requires_grad=True)  # statistics in the graph: only the composition differentiates
    unchanged("log_prob", z, pg)
    unchanged("log_prob", z, p)
    bn._last_mean = keep
    # U = 16 stays with the 16-unit families, U = 17 is the first of the new ones
    for U, rows, train in ((15, "context_rows", "train_context"), (16, "context_rows", "train_context"),
                           (17, ROWS[0], TRAIN[0]), (64, ROWS[0], TRAIN[0])):
        f, q = _flow(5, 2, 2, U)
        f.wide_context_rows = f.wide_context_training = f.context_rows = f.context_training = True
        with torch.no_grad():
            assert f._route("log_prob", z, q).family == rows and f._route("forward", z, q).family == rows
        assert f._route("log_prob", z, q.clone().requires_grad_()).family == train
        f.context_rows = f.context_training = False
        with torch.no_grad():
            assert f._route("log_prob", z, q).family == (rows if U > 16 else "bijectors")
    # the predicates decide: depth and LDS
    for (D, L, U, N), rows, train in (((64, 3, 64, 31), True, False), ((64, 3, 64, 22), True, True), ((64, 3, 64, 23), True, False), ((64, 3, 48, 31), True, True),
                                      ((5, 4, 20, 8), True, False), ((33, 5, 49, 8), False, False), ((32, 5, 64, 8), True, False),
                                      ((5, 6, 20, 8), False, False), ((64, 2, 64, 2), True, True)):
        f, q = _flow(D, 1, L, U)
        f.wide_context_rows = f.wide_context_training = True
        zz = torch.zeros(5, N, D)
        with torch.no_grad():
            assert (f._route("log_prob", zz, q) == ROWS) == rows, (D, L, U, N)
        assert (f._route("log_prob", zz, q.clone().requires_grad_()) == TRAIN) == train, (D, L, U, N)
    # D = 64, N <= 5: the 16-unit family's measured exception is not copied
    d64, q64 = _flow(64, 1, 2, 20)
    d64.wide_context_rows = True
    with torch.no_grad():
        assert d64._route("log_prob", torch.zeros(5, 1, 64), q64) == ROWS
        assert d64._route("forward", torch.zeros(5, 1, 64), q64) == ROWS
    # the measured exclusion, one sample per context above 48 units: today's route
    every = ("log_prob", "inverse", "forward")
    for D, U, N, ops in ((64, 64, 1, ()), (4, 49, 1, ()), (4, 48, 1, every), (4, 20, 1, every), (64, 20, 1, every),
                         (4, 64, 2, every), (64, 64, 31, every)):
        f, q = _flow(D, 2, 2, U)
        zz = torch.zeros(5, N, D)
        with torch.no_grad():
            off = {op: f._route(op, zz, q) for op in ("log_prob", "inverse", "forward")}
            f.wide_context_rows = True
            for op in off:
                assert f._route(op, zz, q) == (ROWS if op in ops else off[op]), (D, U, N, op)
        f.wide_context_training = True  # training has no exclusion: 2.3 x and more in every measured cell
        assert f._route("log_prob", zz, q.clone().requires_grad_()) == TRAIN
    ar, pa = _flow(5, 1, 2, 20, arch="AR")
    ar.wide_context_rows = ar.wide_context_training = True
    with torch.no_grad():
        assert ar._route("log_prob", z, pa).family not in (ROWS[0], TRAIN[0])
    assert ar._route("log_prob", z, pa.clone().requires_grad_()).family not in (ROWS[0], TRAIN[0])
    sup, ps = _flow(5, 2, 2, 20, support_layer=tnf.ToInterval(5, [-1.0] * 5, [2.0] * 5))
    sup.wide_context_rows = sup.wide_context_training = True
    with torch.no_grad():
        assert sup._route("log_prob", z, ps) == ROWS and sup._route("forward", z, ps) == ROWS  # its own kernel
        assert sup._route("inverse", z, ps).family == "bijectors"
    assert sup._route("log_prob", z, ps.clone().requires_grad_()) == TRAIN


def test_routing_table_names_both_families():
    doc = tnf.density_estimator.__doc__
    assert "context_rows_" in doc and "train_context_" in doc and "wide_context_rows" in doc and "wide_context_training" in doc
