"""Training per-context coupling flows with fewer than 32 draws per context through their frozen-statistics samples: one
launch forward, one launch backward (include/tnf_ctxsample.h, csrc/flow_ctx_sample_bwd.hip, NormFlow's family
`train_context_sample`) against float64 autograd through the CPU oracle's composition on float64 copies of the same
float32 inputs (tests/ctxsample_restatement.py `reference`).  Inputs are those of tests/test_gpu_ctx_flow.py (`inputs`,
its z as the draw) plus upstream gradients g_z (M, N, D) and g_sld (M, N) ~ N(0, 1).  Errors are conftest.grad_err -- the
largest error relative to the gradient's largest entry -- and the same per context row, relative to that row's largest
entry; the bars are BAR_P and BAR_Z of tests/domain_helpers.py.  The launch counters check that a step is ONE launch of
the per-context sampling kernel and ONE of the backward kernel and nothing else."""
import numpy as np
import pytest
import torch

import ctxsample_restatement as R
import domain_helpers as H
import test_gpu_ctx_flow as CF
from conftest import grad_err
from domain_helpers import BAR_P, BAR_Z, float64
from test_gpu_ctx_flow import inputs
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
WG = 4  # contexts (waves) per workgroup of the backward kernel at most: ctxsample_ops.WAVES_PER_WORKGROUP


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def cs(tnf):
    from torch_nf_amd import ctxsample_ops

    assert ctxsample_ops.WAVES_PER_WORKGROUP == WG
    return ctxsample_ops


def counters():
    """[launches of the per-context log_prob kernel, of its sampling kernel, of the log_prob backward, of the sampling
    backward]"""
    torch.cuda.synchronize()
    return CF.ctx_counts() + [lib.tnf_ctx_train_launch_count(), lib.tnf_ctx_sample_launch_count()]


class launches(object):
    """`with launches(fwd, bwd)`: the block moves the per-context sampling counter by fwd, the new backward counter by
    bwd, the log_prob counter and the log_prob backward's not at all, and no diag family."""

    def __init__(self, fwd, bwd):
        self.want = [0, fwd, 0, bwd]

    def __enter__(self):
        self.before, self.diag = counters(), H.counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(counters(), self.before)] == self.want
            assert H.launched(self.diag) == {}
        return False


def check(tag, gp, go, want):
    for name, got, ref, bar in (("params", gp, want[0], BAR_P), ("omega", go, want[1], BAR_Z)):
        if got is None:
            continue
        whole, rows = grad_err("ctx_sample %s %s" % (tag, name), got, ref), R.row_err(got, ref)
        print("ctx_sample %s %s: whole %.3e per row %.3e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


def step(cs, omega, params, mean, alpha, g_z, g_sld, shape, o_grad=True):
    """One forward + backward through the autograd entry on the device -> (z, sld, g_params, g_omega | None).  A None
    upstream gradient: that output takes no part in the backward."""
    pc, oc = params.cuda().requires_grad_(), omega.cuda().requires_grad_(o_grad)
    z, sld = cs.ctx_flow_sample_train(oc, pc, mean.cuda(), alpha.cuda(), *shape)
    outs = [(t, g.cuda()) for t, g in ((z, g_z), (sld, g_sld)) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    return z.detach(), sld.detach(), pc.grad, oc.grad


def case(cs, oracle, D, S, L, U, M, N):
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    with launches(1, 1):
        _, _, gp, go = step(cs, omega, params, mean, alpha, g_z, g_sld, shape)
    assert gp.shape == params.shape and go.shape == omega.shape
    check("D=%d S=%d L=%d U=%d M=%d N=%d" % (D, S, L, U, M, N), gp, go,
          R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=(D, S, L, U, M, N)))


# ---- the domain, through the ops entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D,S,L,U,M,N", R.WIDTHS_AND_SAMPLES, ids=lambda v: str(v))
def test_widths_and_samples(cs, oracle, D, S, L, U, M, N):
    """Both parities of D, h = 1, the widths on either side of 32, one sample, 16 and its neighbours, 31; M = 5 is a
    partial last workgroup."""
    case(cs, oracle, D, S, L, U, M, N)


@pytest.mark.parametrize("D,S,L,U,M,N", R.DEPTH_AND_UNITS, ids=lambda v: str(v))
def test_depth_and_units(cs, oracle, D, S, L, U, M, N):
    case(cs, oracle, D, S, L, U, M, N)


@pytest.mark.parametrize("D,S,L,U,M,N", R.WORKGROUP_EDGES, ids=lambda v: str(v))
def test_workgroup_edges(cs, oracle, D, S, L, U, M, N):
    case(cs, oracle, D, S, L, U, M, N)


@pytest.mark.parametrize("D,S,L,U,M,N", R.LARGEST_SLICE, ids=lambda v: str(v))
def test_largest_slice(cs, oracle, D, S, L, U, M, N):
    """49,280 bytes per context: one context per workgroup, served by all its waves."""
    case(cs, oracle, D, S, L, U, M, N)


@pytest.mark.parametrize("o_grad", [False, True])
@pytest.mark.parametrize("which", ["g_z", "g_sld"])
def test_one_upstream_gradient_at_a_time(cs, oracle, which, o_grad):
    """Only z, or only the summed log-det, enters the loss: the other cotangent is absent (NULL for the kernel), with and
    without a gradient for the draw."""
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 17
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    g_z, g_sld = (g_z, None) if which == "g_z" else (None, g_sld)
    shape = (D, S, L, U)
    with launches(1, 1):
        _, _, gp, go = step(cs, omega, params, mean, alpha, g_z, g_sld, shape, o_grad=o_grad)
    assert (go is not None) == o_grad
    check("%s only, omega grad %s" % (which, o_grad), gp, go,
          R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=(which, D, N)))
    # the raw entry with the absent cotangent as explicit zeros: the same bits
    z = cs.ctx_flow_sample_train(omega.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), *shape)[0]
    zeros = (g_z, torch.zeros(M, N)) if which == "g_z" else (torch.zeros(M, N, D), g_sld)
    gp0, go0 = cs.ctx_flow_sample_bwd_raw(z, params.cuda(), mean.cuda(), alpha.cuda(), zeros[0].cuda(), zeros[1].cuda(), *shape)
    assert torch.equal(gp0, gp) and (go is None or torch.equal(go0, go))


def test_longer_rows(cs, oracle):
    """A row stride beyond the parameter count with NaN behind it -- never read, the trailing gradient columns exactly
    zero -- and the gradient columns of the parameters the bits of the plain call."""
    D, S, L, U, M, N = 7, 2, 2, 15, 5, 4
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    P = params.shape[1]
    _, _, gp_plain, go_plain = step(cs, omega, params, mean, alpha, g_z, g_sld, shape)
    wide = torch.full((M, P + 7), float("nan"))
    wide[:, :P] = params
    with launches(1, 1):
        _, _, gp, go = step(cs, omega, wide, mean, alpha, g_z, g_sld, shape)  # pstride = P + 7
    assert gp.shape == (M, P + 7) and not gp[:, P:].any()
    assert torch.equal(gp[:, :P], gp_plain) and torch.equal(go, go_plain)
    check("longer rows", gp[:, :P], go, R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape))


# ---- bitwise properties --------------------------------------------------------------------------------------------------
def test_reproducible(cs, oracle):
    D, S, L, U, M, N = 33, 2, 2, 15, 9, 17
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    a = step(cs, omega, params, mean, alpha, g_z, g_sld, shape)
    b = step(cs, omega, params, mean, alpha, g_z, g_sld, shape)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("D,S,L,U,M,N", [(6, 2, 2, 15, 6, 5), (64, 1, 3, 16, 3, 31)], ids=lambda v: str(v))
def test_rows_stay_with_their_contexts(cs, oracle, D, S, L, U, M, N):
    """Context m's gradients are those of a call with that context alone, bit for bit (one wave per context, and one
    workgroup per context)."""
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N, seed=3)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    _, _, gp, go = step(cs, omega, params, mean, alpha, g_z, g_sld, shape)
    for m in range(M):
        one = slice(m, m + 1)
        _, _, gp1, go1 = step(cs, omega[one], params[one], mean, alpha, g_z[one], g_sld[one], shape)
        assert torch.equal(gp[one], gp1) and torch.equal(go[one], go1), m


def test_forward_is_the_inference_route_bit_for_bit(tnf, cs, oracle):
    from torch_nf_amd import ctxflow_ops

    for D, S, L, U, M, N in ((5, 2, 2, 15, 5, 17), (64, 4, 2, 15, 5, 8)):
        params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
        args = (mean.cuda(), alpha.cuda(), D, S, L, U)
        z_i, sld_i = ctxflow_ops.ctx_flow_forward_raw(omega.cuda(), params.cuda(), *args)
        z, sld = cs.ctx_flow_sample_train(omega.cuda(), params.cuda().requires_grad_(), *args)
        assert z.requires_grad and sld.requires_grad
        assert torch.equal(z.detach(), z_i) and torch.equal(sld.detach(), sld_i)


def test_no_samples_no_launch(cs, oracle):
    D, S, L, U, M = 5, 2, 2, 15, 3
    params, mean, alpha, _ = inputs(oracle, D, S, L, U, M, 8)
    with launches(0, 0):
        gp, go = cs.ctx_flow_sample_bwd_raw(torch.zeros(M, 0, D).cuda(), params.cuda(), mean.cuda(), alpha.cuda(),
                                            torch.zeros(M, 0, D).cuda(), torch.zeros(M, 0).cuda(), D, S, L, U)
    assert gp.shape == params.shape and not gp.any() and go.shape == (M, 0, D)


# ---- through NormFlow and ConditionalDensityEstimator ---------------------------------------------------------------
def test_launches_and_other_routes(tnf, oracle):
    """Switch on: one forward launch, one backward launch, no diag family, log_q formed as on `context_rows`.  Switch off,
    N = 32 or no_grad: the new counter does not move and the results are those of today's routes, bit for bit."""
    D, S, L, U, M = 5, 2, 2, 15, 5
    nf, params, mean, alpha, _ = CF.make_nf(tnf, oracle, D, S, L, U, M, 32)
    nf.context_rows = False
    omega = inputs(oracle, D, S, L, U, M, 32)[3]
    g_z, g_sld = R.upstream(M, 32, D)

    def nf_step(om, gz, gl):
        pc = params.cuda().requires_grad_()
        z, log_q = nf._forward_from(om.cuda(), pc, freeze_bn=True)
        torch.autograd.backward([z, log_q], [gz.cuda(), -gl.double().cuda()])  # log_q = log N(omega) - sld
        return z.detach(), log_q.detach(), pc.grad

    def switched(value, fn):
        nf.context_sample_training = value
        try:
            return fn()
        finally:
            nf.context_sample_training = False

    o8, gz8, gl8 = omega[:, :8].contiguous(), g_z[:, :8].contiguous(), g_sld[:, :8].contiguous()
    with launches(1, 1):
        z_on, lq_on, gp_on = switched(True, lambda: nf_step(o8, gz8, gl8))
    check("NormFlow", gp_on, None, R.reference(oracle, float64, o8, params, mean, alpha, gz8, gl8, (D, S, L, U)))
    before = counters()
    z_off, lq_off, gp_off = nf_step(o8, gz8, gl8)
    assert counters() == before
    torch.testing.assert_close(z_on, z_off, **H.ZF_TOL)
    torch.testing.assert_close(lq_on, lq_off, **H.LQ_TOL)
    grad_err("ctx_sample vs today's route params", gp_on, gp_off, BAR_P)
    nf.context_rows = True  # the inference route's z and log_q, bit for bit
    with torch.no_grad():
        z_i, lq_i = nf._forward_from(o8.cuda(), params.cuda(), freeze_bn=True)
    nf.context_rows = False
    assert torch.equal(z_on, z_i) and torch.equal(lq_on, lq_i)
    before = counters()
    on, off = switched(True, lambda: nf_step(omega, g_z, g_sld)), nf_step(omega, g_z, g_sld)  # N = 32
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    grad_err("ctx_sample N = 32, today's route twice", on[2], off[2], BAR_P)  # (its backward sums with atomics)
    with torch.no_grad():
        on = switched(True, lambda: nf._forward_from(o8.cuda(), params.cuda().requires_grad_(), freeze_bn=True))
        off = nf._forward_from(o8.cuda(), params.cuda().requires_grad_(), freeze_bn=True)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert counters() == before


def _cde(tnf, D, S, H_, seed, support=None):
    """domain_helpers._cde with an optional support layer; with one, the last Affine's log-scales are lowered by 2.5 so
    that the core's samples stay inside the range where a float32 ToInterval resolves its tanh (as in
    tests/test_gpu_sample_train.py)."""
    torch.manual_seed(seed)
    nf = tnf.NormFlow(D, True, "coupling", S, 2, 15, support_layer=support)
    cde = tnf.ConditionalDensityEstimator(nf, 8, [H_])
    g = torch.Generator().manual_seed(seed)
    for b in nf._bn_layers():
        b.set_last_stats(torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) * 0.5 + 0.75)
    with torch.no_grad():
        for p in cde.param_net.parameters():
            p.mul_(0.5)
        if support is not None:
            cde.param_net[-1].bias[-2 * D:-D] -= 2.5
    cde.cuda()
    return nf, cde


@pytest.mark.parametrize("D,sup", [(4, False), (64, False), (4, True)], ids=["D=4", "D=64", "D=4,ToInterval"])
def test_through_the_estimator(tnf, oracle, D, sup):
    """z, log_q = cde(x, 8, freeze_bn=True); loss = sum z^2 + sum log_q: one forward and one backward launch; param_net's
    gradients against the same call with the switch off and against float64 autograd through the float64 copy of the net
    and the oracle.  With a ToInterval support layer the core route is the same and the layer runs behind it."""
    S, M, N = (1 if D == 4 else 4), 6, 8
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    nf, cde = _cde(tnf, D, S, 100 if D == 4 else 32, seed=D, support=tnf.ToInterval(D, lb, ub) if sup else None)
    x = torch.randn(M, 8, generator=torch.Generator().manual_seed(D))

    def grads():
        cde.param_net.zero_grad(set_to_none=True)
        np.random.seed(17)
        z, log_q = cde(x.cuda(), N, freeze_bn=True)
        ((z ** 2).sum() + log_q.sum()).backward()
        return z.detach(), [p.grad.clone() for p in cde.param_net.parameters()]

    before = counters()
    z_off, off = grads()
    assert counters() == before
    nf.context_sample_training = True
    with launches(1, 1):
        z_on, on = grads()
    np.random.seed(17)
    omega = np.random.normal(0.0, 1.0, (M, N, D))  # the draw cde made
    net64 = H._net64(cde)
    with float64():
        z64, lq64, _ = oracle.flow_forward(omega, net64(x.double()), D, S, 2, 15, bn_stats=H._stats64_of(nf))
        if sup:
            z64, ld = oracle.to_interval(z64, tuple(c.double() for c in oracle.interval_consts(lb, ub)), False)
            lq64 = lq64 - ld
        ((z64 ** 2).sum() + lq64.sum()).backward()
    torch.testing.assert_close(z_on.cpu().double(), z64.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(z_on, z_off, rtol=1e-4, atol=1e-4)
    for i, (a, b, w) in enumerate(zip(on, off, net64.parameters())):
        e_today, e_ref = grad_err("ctx_sample cde D=%d sup=%s p%d vs today" % (D, sup, i), a, b), grad_err(
            "ctx_sample cde D=%d sup=%s p%d vs float64" % (D, sup, i), a, w.grad)
        print("ctx_sample cde D=%d sup=%s param %d: vs today's route %.3e, vs float64 %.3e" % (D, sup, i, e_today, e_ref))
        assert e_today <= BAR_P and e_ref <= BAR_P
