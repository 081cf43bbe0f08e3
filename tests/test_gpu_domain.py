"""The narrow coupling kernels (D = 32 / 64, L <= 3, U <= 16) over the whole (D, L, num_stages) domain the library
accepts, against the CPU oracle run in float64 on float64 copies of the same float32 inputs (parameters, frozen
BatchNorm statistics, z or omega) -- so the comparison measures the kernel's error alone, not the oracle's own float32
noise.

The stage counts are derived from the library's own predicates (tnf_flow_fused_supported, tnf_flow_fused2_supported,
tnf_flow_train_rev_supported), scanning S upward, so the sweep follows the LDS layouts when they change; the values
themselves are pinned host-side in tests/test_cabi.py.  Every case names the kernel family it expects in its id and
checks it through the launch counters (tnf_diag_launch_count): where a shape silently moves to another kernel -- the
run-time stage loop of flow_fused_f16 between the flow_fused2 and whole-flow limits, the per-layer chain above the
whole-flow limit, the layer backward above the reversible one -- the move is an explicit expectation.

Tolerances are the suite's existing bars for the same quantities (tests/test_gpu_parity.py, tests/test_gpu_grad.py,
tests/test_gpu_cond.py); none is new."""
import math

import numpy as np
import pytest
import torch

from conftest import grad_err
from domain_helpers import (BAR_P, BAR_Z, FORWARD_FAMILIES, INV_TOL, LOGP_TOL, LQ_TOL, SLDF_TOL, ZF_TOL, _cde, _net64,
                            _stats64_of, counts, float64, launched, variants)
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib

FAMILY_NAMES = {
    L_.DIAG_BWD_LAYER_FP32: "coupling_bwd_mfma", L_.DIAG_BWD_LAYER_F16: "coupling_bwd_f16",
    L_.DIAG_BWD_GENERIC: "coupling_backward", L_.DIAG_BWD_FLOW_REV: "flow_bwd_f16",
    L_.DIAG_MAF_BWD_MFMA: "maf_bwd_mfma", L_.DIAG_MAF_BWD_GENERIC: "maf_backward", L_.DIAG_BWD_WIDE: "coupling_wide_bwd",
    L_.DIAG_FLOW_FUSED2: "flow_fused2", L_.DIAG_FLOW_FUSED2_FWD: "flow_fused2_fwd", L_.DIAG_FLOW_FUSED3: "flow_fused3",
    L_.DIAG_FLOW_F16: "flow_fused_f16", L_.DIAG_FLOW_FP32: "flow_fused", L_.DIAG_FLOW_RANGE2: "flow_range2",
    L_.DIAG_FLOW_RANGE2_FWD: "flow_range2_fwd", L_.DIAG_COUPLING_MFMA: "coupling_mfma", L_.DIAG_COND_FLOW: "cond_flow",
}


# ---- the domain, from the library's predicates --------------------------------------------------------------------
def _s_max(pred, D, L, U=15):
    S = 0
    while pred(D, S + 1, L, U):
        S += 1
    return S


DL = [(D, L) for D in (32, 64) for L in (1, 2, 3)]
S_FLOW = {dl: _s_max(lib.tnf_flow_fused_supported, *dl) for dl in DL}    # whole-flow entry points
S_FUSED2 = {dl: _s_max(lib.tnf_flow_fused2_supported, *dl) for dl in DL}  # the default whole-flow kernel
S_REV = {dl: _s_max(lib.tnf_flow_train_rev_supported, *dl) for dl in DL}  # one-kernel reversible backward


def _stages(D, L):
    return sorted({1, 3, 4, S_FUSED2[D, L], S_FLOW[D, L], S_FLOW[D, L] + 1})


def _units(S):
    return 16 if S == 3 else 15  # U = 16 (no padded unit) once per (D, L)


GRID = [(D, L, S, _units(S)) for D, L in DL for S in _stages(D, L)]

# (kind, variant): TNF_FUSE_FLOW under a flow variant, TNF_FUSE_LAYER under a layer variant, TNF_FUSE_AUTO at the defaults
MODES = [("flow", 10), ("flow", 20), ("flow", 15), ("flow", 0), ("layer", 10), ("layer", 12), ("layer", 13), ("layer", 0),
         ("auto", None)]


def expect_inverse(kind, variant, D, S, L, U):
    """{family: launches} that tnf_flow_log_prob_f32 must enqueue, or None where it must refuse (TnfError)."""
    whole = lib.tnf_flow_fused_supported(D, S, L, U) == 1
    if kind == "auto":
        kind, variant = ("flow", 10) if whole else ("layer", 10)
    if kind == "flow":
        if not whole:
            return None
        if variant == 0:
            return {L_.DIAG_FLOW_FP32: 1}
        if variant == 20 and lib.tnf_flow_fused3_supported(D, S, L, U):
            return {L_.DIAG_FLOW_FUSED3: 1}
        if variant in (10, 20) and lib.tnf_flow_fused2_supported(D, S, L, U):
            return {L_.DIAG_FLOW_FUSED2: 1}
        return {L_.DIAG_FLOW_F16: 1}
    if variant == 0:
        return {L_.DIAG_COUPLING_MFMA: 2 * S}
    per_launch = 1 if variant == 10 else variant - 10
    return {L_.DIAG_FLOW_RANGE2: -(-2 * S // per_launch)}


def expect_forward(kind, D, S, L, U):
    """(families, log_q written by the kernel) of tnf_flow_forward(_logq)_f32 at the default variants."""
    if kind == "layer":
        return {L_.DIAG_FLOW_RANGE2_FWD: 2 * S}, False
    if not lib.tnf_flow_fused_supported(D, S, L, U):
        return None, False
    if lib.tnf_flow_fused2_supported(D, S, L, U):
        return {L_.DIAG_FLOW_FUSED2_FWD: 1}, True
    return {L_.DIAG_FLOW_F16: 1}, False


def _name(fams):
    return "refused" if fams is None else "+".join("%s*%d" % (FAMILY_NAMES[f], n) for f, n in sorted(fams.items()))


def _mode_id(kind, variant):
    return kind if variant is None else "%s%d" % (kind, variant)


INVERSE_CASES = [pytest.param(D, L, S, U, kind, v, id="D%d-L%d-S%d-U%d-%s-%s" % (D, L, S, U, _mode_id(kind, v),
                                                                                 _name(expect_inverse(kind, v, D, S, L, U))))
                 for D, L, S, U in GRID for kind, v in MODES]
FORWARD_CASES = [pytest.param(D, L, S, U, kind, id="D%d-L%d-S%d-U%d-%s-%s" % (D, L, S, U, kind,
                                                                              _name(expect_forward(kind, D, S, L, U)[0])))
                 for D, L, S, U in GRID for kind in ("flow", "layer")]


def test_grid_names_the_fallback_rows():
    """The rows between the flow_fused2 and whole-flow limits run flow_fused_f16 under the default variant: the sweep
    holds them and expects exactly that kernel."""
    for D, L, S in ((64, 2, 7), (64, 3, 6), (32, 3, 9)):
        assert (D, L, S, 15) in GRID
        assert expect_inverse("flow", 10, D, S, L, 15) == {L_.DIAG_FLOW_F16: 1}
        assert expect_forward("flow", D, S, L, 15) == ({L_.DIAG_FLOW_F16: 1}, False)
    assert S_REV[64, 2] == 4 and S_REV[64, 3] == 3  # the headline shape (64, S = 4, L = 2) is the reversible limit


# ---- helpers ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


def flow_inputs(D, S, L, U, Mz, Mp, N, seed):
    """float32 inputs in the pattern of test_gpu_parity._rand_flow: parameter rows, frozen statistics, samples.

    Beyond 4 stages the spread of the random parameters and statistics shrinks as sqrt(4 / S), so that the whole flow
    scales its input about as much as the 4-stage flows of the rest of the suite do.  With the 4-stage spread at every
    depth the 2S random BatchNorm scales compound: at D = 32, L = 1, S = 17 the inverse then maps N(0, 1) samples to
    |z0| ~ 400-1000 and log_prob ~ -1e5, a problem so ill-conditioned that the float32 oracle itself is 3-5e-6 off the
    float64 one -- half the log_prob bar spent on the inputs, not on the kernel."""
    rng = np.random.RandomState(seed)
    k = min(1.0, math.sqrt(4.0 / S))
    P = lib.tnf_flow_num_params(D, S, L, U)
    params = torch.from_numpy(rng.normal(0.0, 0.1 * k, (Mp, P)).astype(np.float32))
    mean = torch.from_numpy(rng.normal(0.0, 0.3 * k, (2 * S, D)).astype(np.float32))
    alpha = torch.from_numpy(np.exp(rng.normal(0.0, 0.2 * k, (2 * S, D))).astype(np.float32))
    z = torch.from_numpy(rng.normal(0.0, 1.0, (Mz, N, D)).astype(np.float32))
    return params, mean, alpha, z


def stats64(mean, alpha):
    return [(m.double(), a.double()) for m, a in zip(mean, alpha)]


_REF = {}


def ref_inverse(oracle, key, z, params, mean, alpha, D, S, L, U):
    """(log_prob, z0, sum_log_det) of the float64 oracle, cached per input set (the modes share it)."""
    if key not in _REF:
        st = stats64(mean, alpha)
        with float64():
            z0, sld = oracle.flow_inverse(z.double(), params.double(), D, S, L, U, st)
            lp = oracle.flow_log_prob(z.double(), params.double(), D, S, L, U, st)
        assert z0.dtype == sld.dtype == lp.dtype == torch.float64
        _REF[key] = (lp, z0, sld)
    return _REF[key]


def check_inverse(tnf, oracle, key, D, S, L, U, kind, variant, params, mean, alpha, z):
    want = expect_inverse(kind, variant, D, S, L, U)
    fusion = {"flow": L_.FUSE_FLOW, "layer": L_.FUSE_LAYER, "auto": L_.FUSE_AUTO}[kind]
    v = dict(flow=variant) if kind == "flow" else (dict(layer=variant) if kind == "layer" else {})
    dev = (z.cuda(), params.cuda(), mean.cuda(), alpha.cuda())
    with variants(**v), torch.no_grad():
        before = counts()
        if want is None:
            with pytest.raises(L_.TnfError) as e:
                tnf.ops.flow_log_prob_raw(*dev, D, S, L, U, fusion, want_z0=True, want_sld=True)
            assert e.value.code == L_.EUNSUPPORTED
            assert launched(before) == {}, "a refused call launched kernels"
            return
        lp, z0, sld = tnf.ops.flow_log_prob_raw(*dev, D, S, L, U, fusion, want_z0=True, want_sld=True)
        ran = launched(before)
    assert ran == want, "ran %s, expected %s" % (_name(ran), _name(want))
    lp_r, z0_r, sld_r = ref_inverse(oracle, key, z, params, mean, alpha, D, S, L, U)
    torch.testing.assert_close(lp.cpu().double(), lp_r, **LOGP_TOL)
    torch.testing.assert_close(z0.cpu().double(), z0_r, **INV_TOL)
    torch.testing.assert_close(sld.cpu().double(), sld_r, **INV_TOL)


# ---- A. inverse / log_prob ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,S,U,kind,variant", INVERSE_CASES)
def test_domain_log_prob(tnf, oracle, D, L, S, U, kind, variant):
    N = 1500
    seed = 1000 * D + 100 * L + S
    params, mean, alpha, z = flow_inputs(D, S, L, U, 1, 1, N, seed)
    check_inverse(tnf, oracle, ("inv", D, L, S, U), D, S, L, U, kind, variant, params, mean, alpha, z)


CONTEXT_MODES = [("flow", 10), ("flow", 15), ("flow", 0), ("layer", 10), ("layer", 13), ("layer", 0)]


@pytest.mark.parametrize("Mz,Mp,N", [(3, 3, 2 * 256 + 17), (3, 1, 2 * 256 + 17), (64, 64, 1100)],
                         ids=["per_context_rows", "broadcast_row", "64_contexts_looping"])
@pytest.mark.parametrize("D,L", DL, ids=["D%d-L%d" % dl for dl in DL])
def test_domain_log_prob_contexts(tnf, oracle, D, L, Mz, Mp, N):
    """Per-context parameter rows, one broadcast row, and M = 64 contexts with N = 1100: the whole-flow grid is then
    capped at ceil(256 / M) workgroups per context, so each workgroup loops over several sample groups.  At the last
    stage count of flow_fused2 (the default kernel's limit), under each family of kernels."""
    S, U = S_FUSED2[D, L], 15
    params, mean, alpha, z = flow_inputs(D, S, L, U, Mz, Mp, N, 7 * D + L + Mz + Mp)
    for kind, v in CONTEXT_MODES:
        check_inverse(tnf, oracle, ("ctx", D, L, S, Mz, Mp, N), D, S, L, U, kind, v, params, mean, alpha, z)


# ---- B. sampling direction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,S,U,kind", FORWARD_CASES)
def test_domain_forward(tnf, oracle, D, L, S, U, kind):
    """ops.flow_forward_raw(..., want_log_q=True), frozen statistics: z, sum_log_det and log_q against the float64
    oracle's flow_forward on the same draw.  log_q comes from the kernel exactly where flow_fused2 holds the shape;
    elsewhere the caller adds the base density on the host side (NormFlow._forward_from), and that value is checked."""
    N = 1500
    params, mean, alpha, _ = flow_inputs(D, S, L, U, 1, 1, 1, 2000 * D + 100 * L + S)
    omega = torch.from_numpy(np.random.RandomState(S).normal(0.0, 1.0, (1, N, D)).astype(np.float32))
    want, lq_from_kernel = expect_forward(kind, D, S, L, U)
    fusion = L_.FUSE_FLOW if kind == "flow" else L_.FUSE_LAYER
    dev = (omega.cuda(), params.cuda(), mean.cuda(), alpha.cuda())
    with torch.no_grad():
        before = counts()
        if want is None:
            with pytest.raises(L_.TnfError) as e:
                tnf.ops.flow_forward_raw(*dev, D, S, L, U, fusion, want_log_q=True)
            assert e.value.code == L_.EUNSUPPORTED
            assert launched(before) == {}, "a refused call launched kernels"
            return
        z, sld, lq = tnf.ops.flow_forward_raw(*dev, D, S, L, U, fusion, want_log_q=True)
        ran = launched(before)
        assert ran == want, "ran %s, expected %s" % (_name(ran), _name(want))
        assert (lq is not None) == lq_from_kernel
        if lq is None:
            lq = tnf.ops.base_log_density_f64(dev[0]) - sld
    with float64():
        z_r, lq_r, _ = oracle.flow_forward(omega.double().numpy(), params.double(), D, S, L, U, stats64(mean, alpha))
    assert z_r.dtype == lq_r.dtype == torch.float64
    sld_r = torch.from_numpy(oracle.base_log_density_f64(omega.double().numpy())) - lq_r
    torch.testing.assert_close(z.cpu().double(), z_r, **ZF_TOL)
    torch.testing.assert_close(sld.cpu().double(), sld_r, **SLDF_TOL)
    torch.testing.assert_close(lq.cpu(), lq_r, **LQ_TOL)


# ---- C. training --------------------------------------------------------------------------------------------------
TRAIN_CASES = [pytest.param(D, L, S, Mp, id="D%d-L%d-S%d-Mp%d-%s" % (D, L, S, Mp, "reversible" if S <= S_REV[D, L] else "layers"))
               for D, L in DL for S in sorted({1, S_REV[D, L], S_REV[D, L] + 1}) for Mp in (1, 3)]


@pytest.mark.parametrize("D,L,S,Mp", TRAIN_CASES)
def test_domain_training(tnf, oracle, D, L, S, Mp):
    """NormFlow.log_prob(z, p) under autograd, z and p requiring grad: the one-kernel reversible backward up to its
    S_max, the layer backward above it; loss and gradients against torch autograd through the float64 oracle."""
    M, N, U = 3, 300, 15
    params, mean, alpha, z_in = flow_inputs(D, S, L, U, M, Mp, N, 3000 * D + 100 * L + 10 * S + Mp)
    w = torch.from_numpy(np.random.RandomState(S + Mp).normal(0.0, 1.0, (M, N)).astype(np.float32))
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    for b, m_, a_ in zip(nf._bn_layers(), mean, alpha):
        b.set_last_stats(m_.cuda(), a_.cuda())
    p, z = params.cuda().requires_grad_(), z_in.cuda().requires_grad_()
    reversible = S <= S_REV[D, L]
    assert nf._train_path(z, p) == ("reversible" if reversible else "layers")
    before = counts()
    loss = (nf.log_prob(z, p) * w.cuda()).sum() / N
    loss.backward()
    ran = launched(before)
    if reversible:  # whole-flow forward keeping z0, one backward kernel (the gated fp32 recovery stays idle)
        assert ran.get(L_.DIAG_FLOW_FUSED2) == 1 and ran.get(L_.DIAG_BWD_FLOW_REV) == 1, _name(ran)
        assert L_.DIAG_BWD_LAYER_F16 not in ran, _name(ran)
    else:  # one fp32-MFMA kernel per layer forward, one split-f16 kernel per layer backward
        assert ran.get(L_.DIAG_COUPLING_MFMA) == 2 * S and ran.get(L_.DIAG_BWD_LAYER_F16) == 2 * S, _name(ran)
        assert L_.DIAG_BWD_FLOW_REV not in ran, _name(ran)
    p_ref, z_ref = params.double().requires_grad_(), z_in.double().requires_grad_()
    with float64():
        loss_ref = (oracle.flow_log_prob(z_ref, p_ref, D, S, L, U, stats64(mean, alpha)) * w.double()).sum() / N
        loss_ref.backward()
    torch.testing.assert_close(loss.detach().cpu().double(), loss_ref.detach(), rtol=1e-5, atol=1e-4)
    path = "reversible pair" if reversible else "per-layer pair"
    grad_err("domain sweep, %s: d params" % path, p.grad, p_ref.grad, BAR_P)
    grad_err("domain sweep, %s: d z" % path, z.grad, z_ref.grad, BAR_Z)


# ---- D. conditional flow ------------------------------------------------------------------------------------------
COND_CASES = [pytest.param(D, L, H, S, id="D%d-L%d-H%d-S%d-cond_flow" % (D, L, H, S))
              for D in (32, 64) for L in (4, 5) for H in (32, 64, 128) for S in (1, 5)]


@pytest.mark.parametrize("D,L,H,S", COND_CASES)
def test_domain_cond_flow_log_prob(tnf, oracle, D, L, H, S):
    M = 300
    nf, cde = _cde(tnf, D, S, L, H, 100 + D + L + H + S)
    x = torch.randn(M, 8, generator=torch.Generator().manual_seed(S))
    z = torch.randn(M, 1, D, generator=torch.Generator().manual_seed(L))
    xd, zd = x.cuda(), z.cuda()
    with torch.no_grad():
        assert cde._fused_conditioner_ok(zd, xd)
        before = counts()
        lp = cde.log_prob(zd, xd)
        assert launched(before, FORWARD_FAMILIES + (L_.DIAG_COND_FLOW,)) == {L_.DIAG_COND_FLOW: 1}
    with torch.no_grad(), float64():
        lp_r = oracle.flow_log_prob(z.double(), _net64(cde)(x.double()), D, S, L, 15, _stats64_of(nf))
    torch.testing.assert_close(lp.cpu().double(), lp_r, **LOGP_TOL)


@pytest.mark.parametrize("D,L,H,S", COND_CASES)
def test_domain_cond_flow_training(tnf, oracle, D, L, H, S):
    """-(w * log_prob).mean() through the fused training pair, in the pattern of test_cond_flow_training_gradients:
    every param_net gradient and the gradient w.r.t. z against torch autograd through the float64 oracle."""
    M = 200
    nf, cde = _cde(tnf, D, S, L, H, 200 + D + L + H + S)
    x = torch.randn(M, 8, generator=torch.Generator().manual_seed(S))
    z0 = torch.randn(M, 1, D, generator=torch.Generator().manual_seed(L))
    w = torch.rand(M, 1, generator=torch.Generator().manual_seed(H)) + 0.1
    z = z0.cuda().requires_grad_()
    assert cde._fused_conditioner_ok(z, x.cuda())
    cde.zero_grad()
    before = counts()
    loss = -(cde.log_prob(z, x.cuda()) * w.cuda()).mean()
    loss.backward()
    assert launched(before, FORWARD_FAMILIES + (L_.DIAG_COND_FLOW,)) == {L_.DIAG_COND_FLOW: 1}
    net = _net64(cde)
    zr = z0.double().requires_grad_()
    with float64():
        loss_r = -(oracle.flow_log_prob(zr, net(x.double()), D, S, L, 15, _stats64_of(nf)) * w.double()).mean()
        loss_r.backward()
    torch.testing.assert_close(loss.detach().cpu().double(), loss_r.detach(), rtol=1e-5, atol=1e-5)

    def close(a, b, tol):
        a, b = a.detach().cpu().double(), b.detach().double()
        scale = float(b.abs().max().clamp_min(1e-30))
        assert float((a - b).abs().max()) <= tol * scale, (float((a - b).abs().max()), scale)

    for a, b in zip(cde.param_net.parameters(), net.parameters()):
        close(a.grad, b.grad, 5e-5)
        grad_err("domain sweep, fused conditioner + flow training, L = 4..5: d param_net", a.grad, b.grad, 1.1e-5)
    close(z.grad, zr.grad, 5e-5)
    grad_err("domain sweep, fused conditioner + flow training, L = 4..5: d z", z.grad, zr.grad, 4e-6)


@pytest.mark.parametrize("D,L,H,S", COND_CASES)
def test_domain_cond_flow_sampling(tnf, oracle, D, L, H, S):
    """cde(x, N = 1, freeze_bn = True) through the fused kernel's sampling direction, in the pattern of
    test_cond_flow_sampling_direction: samples and log-density against the float64 oracle on the same host draw."""
    M = 300
    nf, cde = _cde(tnf, D, S, L, H, 300 + D + L + H + S)
    x = torch.randn(M, 8, generator=torch.Generator().manual_seed(S))
    xd = x.cuda()
    with torch.no_grad():
        assert cde._fused_sampling_ok(xd)
        np.random.seed(7)
        before = counts()
        z, lq = cde(xd, N=1, freeze_bn=True)
        assert launched(before, FORWARD_FAMILIES + (L_.DIAG_COND_FLOW,)) == {L_.DIAG_COND_FLOW: 1}
    np.random.seed(7)
    omega = np.random.normal(0.0, 1.0, (M, 1, D))
    with torch.no_grad(), float64():
        z_r, lq_r, _ = oracle.flow_forward(omega, _net64(cde)(x.double()), D, S, L, 15, _stats64_of(nf))
    torch.testing.assert_close(z.cpu().double(), z_r, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(lq.cpu().double(), lq_r, rtol=1e-5, atol=1e-4)
