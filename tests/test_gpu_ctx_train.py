"""Training per-context coupling flows with fewer than 32 samples per context: one launch forward, one launch backward
(include/tnf_ctxtrain.h, csrc/flow_ctx_bwd.hip, NormFlow's family `train_context`) against float64 autograd through the
CPU oracle on float64 copies of the same float32 inputs.  Inputs are those of tests/test_gpu_ctx_flow.py (`inputs`) plus
an upstream gradient ~ N(0, 1) of shape (M, N).  Errors are conftest.grad_err -- the largest error relative to the
gradient's largest entry -- and the same per context row, relative to that row's largest entry; the bars are BAR_P and
BAR_Z of tests/test_gpu_grad.py (4 x the errors measured for the reversible pair).  The launch counters check that a
step is ONE launch of the forward kernel and ONE of the backward kernel and nothing else."""
import numpy as np
import pytest
import torch

import domain_helpers as H
import test_gpu_ctx_flow as CF
from conftest import grad_err
from domain_helpers import BAR_P, BAR_Z, float64
from test_gpu_ctx_flow import inputs, st64
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
WG = 4  # contexts (waves) per workgroup of the backward kernel at most: ctxtrain_ops.WAVES_PER_WORKGROUP


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def ct(tnf):
    from torch_nf_amd import ctxtrain_ops

    assert ctxtrain_ops.WAVES_PER_WORKGROUP == WG
    return ctxtrain_ops


def counters():
    """[forward launches of the per-context log_prob kernel, its sampling launches, backward launches]"""
    torch.cuda.synchronize()
    return CF.ctx_counts() + [lib.tnf_ctx_train_launch_count()]


class launches(object):
    """`with launches(fwd, bwd)`: the block moves the per-context log_prob counter by fwd, the backward counter by bwd,
    the sampling counter not at all, and no diag family."""

    def __init__(self, fwd, bwd):
        self.want = [fwd, 0, bwd]

    def __enter__(self):
        self.before, self.diag = counters(), H.counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(counters(), self.before)] == self.want
            assert H.launched(self.diag) == {}
        return False


def upstream(M, N, seed=0):
    return torch.randn(M, N, generator=torch.Generator().manual_seed(77 + 100 * M + N + seed))


_REF = {}


def reference(oracle, z, params, mean, alpha, g, shape, key=None):
    """(g_params, g_z) float64: autograd through oracle.flow_log_prob on float64 copies; computed once per `key`."""
    if key is None or key not in _REF:
        with float64():
            p64, z64 = params.double().requires_grad_(), z.double().requires_grad_()
            lp = oracle.flow_log_prob(z64, p64, *shape, st64(mean, alpha))
            (lp * g.double()).sum().backward()
        if key is None:
            return p64.grad, z64.grad
        _REF[key] = (p64.grad, z64.grad)
    return _REF[key]


def row_err(got, want):
    """The largest error of a context's row relative to that row's largest entry, over the contexts."""
    got, want = got.detach().double().cpu().flatten(1), want.detach().double().cpu().flatten(1)
    return float(((got - want).abs().max(1).values / want.abs().max(1).values.clamp_min(1e-300)).max())


def check(tag, gp, gz, want):
    for name, got, ref, bar in (("params", gp, want[0], BAR_P), ("z", gz, want[1], BAR_Z)):
        if got is None:
            continue
        whole, rows = grad_err("ctx_train %s %s" % (tag, name), got, ref), row_err(got, ref)
        print("ctx_train %s %s: whole %.3e per row %.3e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


def step(ct, z, params, mean, alpha, g, shape, z_grad=True):
    """One forward + backward through the autograd entry on the device -> (log_prob, g_params, g_z | None)."""
    pc, zc = params.cuda().requires_grad_(), z.cuda().requires_grad_(z_grad)
    lp = ct.ctx_flow_log_prob_train(zc, pc, mean.cuda(), alpha.cuda(), *shape)
    lp.backward(g.cuda())
    return lp.detach(), pc.grad, zc.grad


def case(ct, oracle, D, S, L, U, M, N):
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    g, shape = upstream(M, N), (D, S, L, U)
    with launches(1, 1):
        _, gp, gz = step(ct, z, params, mean, alpha, g, shape)
    assert gp.shape == params.shape and gz.shape == z.shape
    check("D=%d S=%d L=%d U=%d M=%d N=%d" % (D, S, L, U, M, N), gp, gz,
          reference(oracle, z, params, mean, alpha, g, shape, key=(D, S, L, U, M, N)))


# ---- the domain, through the ops entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 31])
@pytest.mark.parametrize("D", [2, 5, 16, 31, 32, 33, 63, 64])
def test_widths_and_samples(ct, oracle, D, N):
    """Both parities of D, h = 1, the widths on either side of 32, one sample, 16 and its neighbours, 31; M = 5 is a
    partial last workgroup."""
    case(ct, oracle, D, 2, 2, 15, 5, N)


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D", [5, 64])
def test_depth_and_units(ct, oracle, D, L, S):
    case(ct, oracle, D, S, L, 16, 3, 7)


@pytest.mark.parametrize("M", [1, WG - 1, WG, WG + 1])
def test_workgroup_edges(ct, oracle, M):
    case(ct, oracle, 6, 2, 2, 15, M, 3)
    case(ct, oracle, 64, 1, 3, 16, M, 31)  # the largest slice: one context per workgroup


def raw(ct, oracle, z, params, mean, alpha, g, shape, want_gz=True):
    """The backward kernel alone on the z0 of the float32 oracle inverse (any z0 serves the bitwise properties)."""
    with torch.no_grad():
        z0, _ = oracle.flow_inverse(z, params[:, :oracle.flow_num_params(*shape)], *shape, list(zip(mean, alpha)))
    return ct.ctx_flow_log_prob_bwd_raw(z0.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), g.cuda(), *shape, want_gz=want_gz)


def test_rows_stay_with_their_contexts(ct, oracle):
    """Context m's gradients are those of a call with that context alone, bit for bit, and a permutation of the contexts
    permutes the gradient rows."""
    D, S, L, U, M, N = 6, 2, 2, 15, 6, 5
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, seed=3)
    g, shape = upstream(M, N), (D, S, L, U)
    gp, gz = raw(ct, oracle, z, params, mean, alpha, g, shape)
    for m in range(M):
        gp1, gz1 = raw(ct, oracle, z[m:m + 1], params[m:m + 1], mean, alpha, g[m:m + 1], shape)
        assert torch.equal(gp[m:m + 1], gp1) and torch.equal(gz[m:m + 1], gz1), m
    perm = torch.tensor([4, 0, 5, 2, 1, 3])
    gp_p, gz_p = raw(ct, oracle, z[perm], params[perm], mean, alpha, g[perm], shape)
    assert torch.equal(gp[perm.cuda()], gp_p) and torch.equal(gz[perm.cuda()], gz_p)


def test_reproducible(ct, oracle):
    D, S, L, U, M, N = 33, 2, 2, 15, 9, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    g, shape = upstream(M, N), (D, S, L, U)
    a, b = step(ct, z, params, mean, alpha, g, shape), step(ct, z, params, mean, alpha, g, shape)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_zero_upstream_gradient(ct, oracle):
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    shape = (D, S, L, U)
    _, gp, gz = step(ct, z, params, mean, alpha, torch.zeros(M, N), shape)
    assert not gp.any() and not gz.any()  # exactly zero everywhere
    g = torch.zeros(M, N)
    g[2, 16] = 1.5  # one sample of one context
    _, gp, gz = step(ct, z, params, mean, alpha, g, shape)
    want = reference(oracle, z, params, mean, alpha, g, shape)
    rows = [m for m in range(M) if m != 2]
    assert not gp[rows].any() and not gz[rows].any() and not gz[2, :16].any()
    check("one sample", gp[2:3], gz[2:3], (want[0][2:3], want[1][2:3]))


def test_longer_rows_and_expanded_views(ct, oracle):
    """A row stride beyond the row with NaN behind it -- never read, the trailing gradient columns exactly zero -- and an
    expanded single row (stride 0): the gradient is the sum over contexts of the per-row gradients of the repeated row."""
    D, S, L, U, M, N = 7, 2, 2, 15, 5, 4
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    g, shape = upstream(M, N), (D, S, L, U)
    P = params.shape[1]
    want = reference(oracle, z, params, mean, alpha, g, shape, key=(D, S, L, U, M, N))
    _, gp_plain, gz_plain = step(ct, z, params, mean, alpha, g, shape)
    wide = torch.full((M, P + 7), float("nan"))
    wide[:, :P] = params
    with launches(1, 1):
        _, gp, gz = step(ct, z, wide, mean, alpha, g, shape)  # pstride = P + 7
    assert gp.shape == (M, P + 7) and not gp[:, P:].any()
    assert torch.equal(gp[:, :P], gp_plain) and torch.equal(gz, gz_plain)
    check("longer rows", gp[:, :P], gz, want)
    big = wide.cuda()
    view = big[:, :P].requires_grad_()
    assert view.stride(0) == P + 7 and not view.is_contiguous()
    ct.ctx_flow_log_prob_train(z.cuda(), view, mean.cuda(), alpha.cuda(), *shape).backward(g.cuda())
    assert torch.equal(view.grad, gp_plain)
    row = params[1:2].cuda().requires_grad_()
    expanded = row.expand(M, P)
    assert expanded.stride(0) == 0
    with launches(1, 1):
        ct.ctx_flow_log_prob_train(z.cuda(), expanded, mean.cuda(), alpha.cuda(), *shape).backward(g.cuda())
    _, gp_rep, _ = step(ct, z, params[1:2].repeat(M, 1), mean, alpha, g, shape)
    torch.testing.assert_close(row.grad, gp_rep.sum(0, keepdim=True), rtol=1e-6, atol=1e-6 * float(gp_rep.abs().max()))
    want_e = reference(oracle, z, params[1:2].repeat(M, 1), mean, alpha, g, shape)[0].sum(0, keepdim=True)
    check("expanded row", row.grad, None, (want_e, None))


def test_outputs_requested(ct, oracle):
    """g_z is None when z does not require grad; a shared block z (1, N, D) that requires no grad runs the new route and
    matches the oracle on the expanded z."""
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 9
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, Mz=1)
    assert z.shape[0] == 1
    g, shape = upstream(M, N), (D, S, L, U)
    with launches(1, 1):
        lp, gp, gz = step(ct, z, params, mean, alpha, g, shape, z_grad=False)
    assert gz is None and lp.shape == (M, N)
    want = reference(oracle, z.expand(M, N, D).contiguous(), params, mean, alpha, g, shape)
    check("shared z", gp, None, want)
    full = inputs(oracle, D, S, L, U, M, N)[3]
    _, gp_a, gz_a = step(ct, full, params, mean, alpha, g, shape)
    _, gp_b, gz_b = step(ct, full, params, mean, alpha, g, shape, z_grad=False)
    assert gz_b is None and gz_a is not None and torch.equal(gp_a, gp_b)
    gp_r, gz_r = raw(ct, oracle, full, params, mean, alpha, g, shape, want_gz=False)
    assert gz_r is None and gp_r.shape == params.shape


def test_no_samples_no_launch(ct, oracle):
    D, S, L, U, M = 5, 2, 2, 15, 3
    params, mean, alpha, _ = inputs(oracle, D, S, L, U, M, 8)
    with launches(0, 0):
        gp, gz = ct.ctx_flow_log_prob_bwd_raw(torch.zeros(M, 0, D).cuda(), params.cuda(), mean.cuda(), alpha.cuda(),
                                              torch.zeros(M, 0).cuda(), D, S, L, U)
    assert gp.shape == params.shape and not gp.any() and gz.shape == (M, 0, D)


# ---- through NormFlow and ConditionalDensityEstimator ---------------------------------------------------------------
def make_nf(tnf, oracle, D, S, L, U, M, N, support=None):
    nf, params, mean, alpha, z = CF.make_nf(tnf, oracle, D, S, L, U, M, N, support=support)
    nf.context_rows = False
    nf.context_training = True
    return nf, params, mean, alpha, z


def nf_step(nf, z, params, g, z_grad=False):
    pc, zc = params.cuda().requires_grad_(), z.cuda().requires_grad_(z_grad)
    lp = nf.log_prob(zc, pc)
    lp.backward(g.cuda())
    return lp.detach(), pc.grad, zc.grad


def test_launches_and_other_routes(tnf, oracle):
    """Switch on: one forward launch, one backward launch, no diag family.  Switch off, N = 32 or no_grad: the new counter
    does not move and the results are those of today's routes, bit for bit."""
    D, S, L, U, M = 5, 2, 2, 15, 5
    nf, params, mean, alpha, _ = make_nf(tnf, oracle, D, S, L, U, M, 32)
    z = inputs(oracle, D, S, L, U, M, 32)[3]
    g = upstream(M, 32)
    with launches(1, 1):
        lp_on, gp_on, gz_on = nf_step(nf, z[:, :8], params, g[:, :8], z_grad=True)
    check("NormFlow", gp_on, gz_on, reference(oracle, z[:, :8], params, mean, alpha, g[:, :8], (D, S, L, U)))

    def today(fn):
        nf.context_training = False
        try:
            return fn()
        finally:
            nf.context_training = True

    before = counters()
    lp_off, gp_off, gz_off = today(lambda: nf_step(nf, z[:, :8], params, g[:, :8], z_grad=True))
    assert counters() == before
    torch.testing.assert_close(lp_on, lp_off, **H.LOGP_TOL)
    grad_err("ctx_train vs today's route params", gp_on, gp_off, BAR_P)
    grad_err("ctx_train vs today's route z", gz_on, gz_off, BAR_Z)
    for a, b in zip(nf_step(nf, z, params, g, z_grad=True), today(lambda: nf_step(nf, z, params, g, z_grad=True))):
        assert torch.equal(a, b)  # N = 32
    with torch.no_grad():
        pg = params.cuda().requires_grad_()
        assert torch.equal(nf.log_prob(z[:, :8].cuda(), pg), today(lambda: nf.log_prob(z[:, :8].cuda(), pg)))
    nf.context_training = False
    plain = nf_step(nf, z[:, :8], params, g[:, :8])
    nf.context_rows = True  # context_rows alone leaves autograd calls on today's route
    for a, b in zip(nf_step(nf, z[:, :8], params, g[:, :8])[:2], plain[:2]):
        assert torch.equal(a, b)
    assert counters() == before


@pytest.mark.parametrize("D", [4, 64])
def test_through_the_estimator(tnf, oracle, D):
    """cde.log_prob(z (M, 8, D), x) under autograd: one forward and one backward launch; param_net's gradients against the
    same call with the switch off and against float64 autograd through the float64 copy of the net and the oracle."""
    S, L, M, N = (1 if D == 4 else 4), 2, 6, 8
    nf, cde = H._cde(tnf, D, S, L, 100 if D == 4 else 32, seed=D)
    gen = torch.Generator().manual_seed(D)
    x, z, g = torch.randn(M, 8, generator=gen), torch.randn(M, N, D, generator=gen), upstream(M, N)

    def grads():
        cde.param_net.zero_grad(set_to_none=True)
        (cde.log_prob(z.cuda(), x.cuda()) * g.cuda()).sum().backward()
        return [p.grad.clone() for p in cde.param_net.parameters()]

    before = counters()
    off = grads()
    assert counters() == before
    nf.context_training = True
    with launches(1, 1):
        on = grads()
    net64 = H._net64(cde)
    with float64():
        lp = oracle.flow_log_prob(z.double(), net64(x.double()), D, S, L, 15, H._stats64_of(nf))
        (lp * g.double()).sum().backward()
    for i, (a, b, w) in enumerate(zip(on, off, net64.parameters())):
        e_today, e_ref = grad_err("ctx_train cde D=%d p%d vs today" % (D, i), a, b), grad_err(
            "ctx_train cde D=%d p%d vs float64" % (D, i), a, w.grad)
        print("ctx_train cde D=%d param %d: vs today's route %.3e, vs float64 %.3e" % (D, i, e_today, e_ref))
        assert e_today <= BAR_P and e_ref <= BAR_P


def test_support_layer_runs_as_its_own_kernel(tnf, oracle):
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 8
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    nf, params, mean, alpha, _ = make_nf(tnf, oracle, D, S, L, U, M, N, support=tnf.ToInterval(D, lb, ub))
    z = torch.from_numpy(np.random.RandomState(0).uniform(-1.5, 2.5, (M, N, D)).astype(np.float32))
    g = upstream(M, N)
    consts = tuple(c.double() for c in oracle.interval_consts(lb, ub))
    before = counters()
    _, gp, gz = nf_step(nf, z, params, g, z_grad=True)
    assert [a - b for a, b in zip(counters(), before)] == [1, 0, 1]  # the core route is the new one
    with float64():
        p64, z64 = params.double().requires_grad_(), z.double().requires_grad_()
        z_in, ld_sup = oracle.to_interval(z64, consts, True)
        lp = oracle.flow_log_prob(z_in, p64, D, S, L, U, st64(mean, alpha)) - ld_sup
        (lp * g.double()).sum().backward()
    check("support layer", gp, gz, (p64.grad, z64.grad))


def test_graph_capture(tnf, oracle):
    """A whole step -- forward, backward, into preallocated .grad -- captured on a single stream (no parallel branches)
    replays to the eager step's bits; the counters do not move on replay."""
    D, S, L, U, M, N = 6, 2, 2, 15, 7, 8
    nf, params, mean, alpha, z = make_nf(tnf, oracle, D, S, L, U, M, N)
    g = upstream(M, N).cuda()
    pc, zc = params.cuda().requires_grad_(), z.cuda()
    pc.grad = torch.zeros_like(pc)

    def one_step():
        pc.grad.zero_()
        lp = nf.log_prob(zc, pc)
        lp.backward(g)
        return lp.detach()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the side stream
            one_step()
    torch.cuda.current_stream().wait_stream(s)
    lp_eager, gp_eager = one_step().clone(), pc.grad.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lp = one_step()
    before = counters()
    pc.grad.fill_(7.0)
    lp.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert counters() == before  # a replay runs the captured kernels; no call reaches the host launchers
    assert torch.equal(lp, lp_eager) and torch.equal(pc.grad, gp_eager)
