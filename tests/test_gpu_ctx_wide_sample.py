"""Training per-context coupling flows with 17 .. 64 units and fewer than 32 draws per context through their
frozen-statistics samples: one launch forward (the wide per-context sampling kernel), one launch backward
(include/tnf_ctxwidesample.h, csrc/flow_ctx_wide_sample_bwd.hip, NormFlow's family `train_context_sample_wide`) against
float64 autograd through the CPU oracle's composition on float64 copies of the same float32 inputs
(tests/ctxsample_restatement.py `reference`).  Inputs are those of tests/test_gpu_ctx_flow.py (`inputs`, its z as the
draw) plus upstream gradients g_z (M, N, D) and g_sld (M, N) ~ N(0, 1).  Errors are conftest.grad_err -- the largest error
relative to the gradient's largest entry -- and the same per context row.

Bars.  BAR_P and BAR_Z of tests/domain_helpers.py per group of cases (tests/ctxwidesample_restatement.py `groups`), unless
the float32 restatement of the walk alone exceeds a quarter of one on the group's own cases: then 4 x the restatement's
error, computed here on the host from the restatement, never from the kernel (`bars`; the rule of
tests/test_gpu_ctx_wide.py).  On the host that wrote profiles/r23_ctxwidesample_grad_errors.json one bar is computed: omega
at S = 9, L = 1 (restatement 6.0e-6 at D = 64, U = 64: the float32 rebuild through 18 one-hidden-layer couplings)."""
import numpy as np
import pytest
import torch

import ctxwidesample_restatement as R
import domain_helpers as H
import test_gpu_ctx_flow as CF
from conftest import grad_err
from domain_helpers import BAR_P, BAR_Z, float64
from test_gpu_ctx_flow import inputs
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def cws(tnf):
    from torch_nf_amd import ctxwidesample_ops

    assert ctxwidesample_ops.TEAMS == R.TEAM_SIZES
    assert lib.tnf_ctx_wide_sample_set_waves(0) == 0  # the automatic choice is the default, and nothing left it changed
    return ctxwidesample_ops


def counters():
    """[launches of the wide per-context sampling kernel, of the new backward]"""
    torch.cuda.synchronize()
    return [lib.tnf_ctx_wide_launch_count(1), lib.tnf_ctx_wide_sample_launch_count()]


def other_counts():
    return (CF.ctx_counts() + [lib.tnf_ctx_train_launch_count(), lib.tnf_ctx_sample_launch_count(),
                               lib.tnf_wide_flow_launch_count(0), lib.tnf_wide_flow_launch_count(1),
                               lib.tnf_ctx_wide_launch_count(0), lib.tnf_ctx_wide_launch_count(2)])


class launches(object):
    """`with launches(fwd, bwd)`: the block moves the wide sampling kernel's counter by fwd and the new backward's by bwd,
    no other counter of the per-context and wide families, and no diag family."""

    def __init__(self, fwd, bwd):
        self.want = [fwd, bwd]

    def __enter__(self):
        self.before, self.others, self.diag = counters(), other_counts(), H.counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(counters(), self.before)] == self.want
            assert other_counts() == self.others and H.launched(self.diag) == {}
        return False


class forced(object):
    """`with forced(waves)`: every backward of the block runs on a team of that size; the previous setting comes back."""

    def __init__(self, waves):
        self.waves = waves

    def __enter__(self):
        self.prev = lib.tnf_ctx_wide_sample_set_waves(self.waves)
        assert self.prev >= 0

    def __exit__(self, *exc):
        assert lib.tnf_ctx_wide_sample_set_waves(self.prev) == self.waves
        return False


def dev(*ts):
    return tuple(t.cuda() for t in ts)


def check(tag, gp, go, want, bars=(BAR_P, BAR_Z)):
    for name, got, ref, bar in (("params", gp, want[0], bars[0]), ("omega", go, want[1], bars[1])):
        if got is None:
            continue
        whole, rows = grad_err("ctx_wide_sample %s %s" % (tag, name), got, ref), R.row_err(got, ref)
        print("ctx_wide_sample %s %s: whole %.3e per row %.3e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


def step(cws, omega, params, mean, alpha, g_z, g_sld, shape, o_grad=True):
    """One forward + backward through the autograd entry on the device -> (z, sld, g_params, g_omega | None).  A None
    upstream gradient: that output takes no part in the backward."""
    pc, oc = params.cuda().requires_grad_(), omega.cuda().requires_grad_(o_grad)
    z, sld = cws.ctx_wide_sample_train(oc, pc, mean.cuda(), alpha.cuda(), *shape)
    outs = [(t, g.cuda()) for t, g in ((z, g_z), (sld, g_sld)) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    return z.detach(), sld.detach(), pc.grad, oc.grad


def run_case(cws, oracle, case):
    D, S, L, U, M, N = case
    params, mean, alpha, omega = inputs(oracle, *case)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    with launches(1, 1):
        _, _, gp, go = step(cws, omega, params, mean, alpha, g_z, g_sld, shape)
    assert gp.shape == params.shape and go.shape == omega.shape
    check(R.case_id(case), gp, go, R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=case),
          R.bars(oracle, R.group_of(case)))
    return gp, go


# ---- the domain, through the ops entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", R.SAMPLES)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_widths_and_samples(cws, oracle, D, N):
    """Both parities of D, h = 1, the widths on either side of 32, one sample, 16 and its neighbours, 31."""
    run_case(cws, oracle, (D, 2, 2, 20, 5, N))


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("D", [5, 64])
@pytest.mark.parametrize("U", [17, 48, 64])
@pytest.mark.parametrize("L", [1, 3])
def test_depth_and_units(cws, oracle, L, U, D, S):
    run_case(cws, oracle, (D, S, L, U, 3, 7))


@pytest.mark.parametrize("case", R.TEAMS_AND_SLICES, ids=R.case_id)
def test_teams_and_slices(cws, oracle, case):
    """The automatic team against the bars, then each forced team: the same bits.  Among the cases: one sample, one
    context, the largest slices at L = 2 and L = 3, the last N that fits at D = 64, L = 3, U = 64."""
    D, S, L, U, M, N = case
    gp, go = run_case(cws, oracle, case)
    params, mean, alpha, omega = inputs(oracle, *case)
    g_z, g_sld = R.upstream(M, N, D)
    assert cws.waves(D, U, N) == R.auto_waves(D, U, N)
    for waves in R.TEAM_SIZES:
        with forced(waves), launches(1, 1):
            _, _, gp_w, go_w = step(cws, omega, params, mean, alpha, g_z, g_sld, (D, S, L, U))
        assert torch.equal(gp_w, gp) and torch.equal(go_w, go), waves
    assert lib.tnf_ctx_wide_sample_set_waves(0) == 0  # restored


def test_automatic_teams_cover_all_three(cws):
    assert {cws.waves(c[0], c[3], c[5]) for c in R.GRID} == set(R.TEAM_SIZES)
    assert {cws.waves(c[0], c[3], c[5]) for c in R.TEAMS_AND_SLICES} == set(R.TEAM_SIZES)
    assert W_LDS(64, 1, 2, 64, 31) == 123008 and W_LDS(33, 1, 3, 64, 31) == 144512


def W_LDS(D, S, L, U, N):
    return lib.tnf_ctx_wide_lds_bytes(1, D, S, L, U, N)


@pytest.mark.parametrize("D,S,L,U,M,N", R.ONE_COTANGENT, ids=lambda v: str(v))
@pytest.mark.parametrize("o_grad", [False, True])
@pytest.mark.parametrize("which", ["g_z", "g_sld"])
def test_one_upstream_gradient_at_a_time(cws, oracle, which, o_grad, D, S, L, U, M, N):
    """Only z, or only the summed log-det, enters the loss: the other cotangent is absent (NULL for the kernel), with and
    without a gradient for the draw."""
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    g_z, g_sld = (g_z, None) if which == "g_z" else (None, g_sld)
    shape = (D, S, L, U)
    with launches(1, 1):
        _, _, gp, go = step(cws, omega, params, mean, alpha, g_z, g_sld, shape, o_grad=o_grad)
    assert (go is not None) == o_grad
    check("%s only, omega grad %s, D=%d" % (which, o_grad, D), gp, go,
          R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=(which, D, S, L, U, M, N)))
    # the raw entry with the absent cotangent as explicit zeros: the same bits
    z = cws.ctx_wide_sample_train(omega.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), *shape)[0]
    zeros = (g_z, torch.zeros(M, N)) if which == "g_z" else (torch.zeros(M, N, D), g_sld)
    gp0, go0 = cws.ctx_wide_sample_bwd_raw(z, params.cuda(), mean.cuda(), alpha.cuda(), zeros[0].cuda(), zeros[1].cuda(),
                                           *shape)
    assert torch.equal(gp0, gp) and (go is None or torch.equal(go0, go))


def test_zero_upstream_gradient_gives_exact_zeros(cws, oracle):
    D, S, L, U, M, N = 5, 2, 2, 20, 5, 17
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    with launches(1, 1):
        _, _, gp, go = step(cws, omega, params, mean, alpha, torch.zeros(M, N, D), torch.zeros(M, N), (D, S, L, U))
    assert not gp.any() and not go.any()
    # a loss that uses neither output: no backward launch at all
    pc = params.cuda().requires_grad_()
    z, sld = cws.ctx_wide_sample_train(omega.cuda(), pc, mean.cuda(), alpha.cuda(), D, S, L, U)
    before = counters()
    (pc * 0).sum().backward()
    assert counters() == before and z.requires_grad and sld.requires_grad


def test_longer_rows(cws, oracle):
    """A row stride beyond the parameter count with NaN behind it -- never read, the trailing gradient columns exactly
    zero -- and the gradient columns of the parameters the bits of the plain call."""
    D, S, L, U, M, N = 7, 2, 2, 20, 5, 4
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    P = params.shape[1]
    _, _, gp_plain, go_plain = step(cws, omega, params, mean, alpha, g_z, g_sld, shape)
    wide = torch.full((M, P + 7), float("nan"))
    wide[:, :P] = params
    with launches(1, 1):
        _, _, gp, go = step(cws, omega, wide, mean, alpha, g_z, g_sld, shape)  # pstride = P + 7
    assert gp.shape == (M, P + 7) and not gp[:, P:].any()
    assert torch.equal(gp[:, :P], gp_plain) and torch.equal(go, go_plain)
    check("longer rows", gp[:, :P], go, R.reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape))


# ---- bitwise properties --------------------------------------------------------------------------------------------------
def test_forward_is_the_inference_route_bit_for_bit(cws, oracle):
    from torch_nf_amd import ctxwide_ops

    for D, S, L, U, M, N in ((5, 2, 2, 20, 5, 17), (64, 1, 3, 48, 3, 31), (4, 1, 2, 20, 5, 1)):
        params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
        args = (mean.cuda(), alpha.cuda(), D, S, L, U)
        z_i, sld_i = ctxwide_ops.ctx_wide_forward_raw(omega.cuda(), params.cuda(), *args)
        with launches(1, 0):
            z, sld = cws.ctx_wide_sample_train(omega.cuda(), params.cuda().requires_grad_(), *args)
        assert z.requires_grad and sld.requires_grad
        assert torch.equal(z.detach(), z_i) and torch.equal(sld.detach(), sld_i)


@pytest.mark.parametrize("D,S,L,U,M,N", [(6, 2, 2, 20, 6, 17), (64, 1, 3, 48, 3, 31)], ids=lambda v: str(v))
def test_rows_stay_with_their_contexts_and_runs_repeat(cws, oracle, D, S, L, U, M, N):
    """Context m's gradient row and g_omega are those of a call with that context alone, bit for bit; a permutation of the
    contexts permutes them; two runs give the same bits."""
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N, seed=3)
    assert len({tuple(r.tolist()) for r in params}) == M  # pairwise different rows
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    got = step(cws, omega, params, mean, alpha, g_z, g_sld, shape)
    for a, b in zip(got, step(cws, omega, params, mean, alpha, g_z, g_sld, shape)):
        assert torch.equal(a, b)
    for m in range(M):
        one = slice(m, m + 1)
        for a, b in zip(got, step(cws, omega[one], params[one], mean, alpha, g_z[one], g_sld[one], shape)):
            assert torch.equal(a[one], b), m
    perm = torch.arange(M - 1, -1, -1) if M < 6 else torch.tensor([4, 0, 5, 2, 1, 3])
    for a, b in zip(got, step(cws, omega[perm], params[perm], mean, alpha, g_z[perm], g_sld[perm], shape)):
        assert torch.equal(a[perm.cuda()], b)


def test_alignment_strides_and_guards(cws, oracle):
    """Rows at 4-byte alignment (every buffer one float off a 16-byte boundary), a parameter and a gradient row stride
    beyond the row with NaN behind the row, and guard values around every output: all intact, same bits as the plain call."""
    D, S, L, U, M, N = 7, 2, 2, 20, 5, 17
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    (g_z, g_sld), shape = R.upstream(M, N, D), (D, S, L, U)
    P, pad = params.shape[1], 7
    z, _, gp, go = step(cws, omega, params, mean, alpha, g_z, g_sld, shape)

    def off(t, cols=None):
        """A copy of t one float past a 16-byte boundary with NaN guards around it -> (view, buffer)."""
        n = t.numel() if cols is None else t.shape[0] * cols
        buf = torch.full((n + 9,), float("nan"), device="cuda")
        if cols is None:
            view = buf[5:5 + n].view(t.shape)
        else:
            view = buf[5:5 + n].view(t.shape[0], cols)[:, :t.shape[1]]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view, buf

    def guards_intact(buf, view, cols=None):
        inside = torch.zeros_like(buf, dtype=torch.bool)
        n = view.numel() if cols is None else view.shape[0] * cols
        region = inside[5:5 + n]
        if cols is None:
            region[:] = True
        else:
            region.view(view.shape[0], cols)[:, :view.shape[1]] = True
        return bool(torch.isnan(buf[~inside]).all()) and not bool(torch.isnan(buf[inside]).any())

    z_v, _ = off(z)
    p_v, _ = off(params.cuda(), cols=P + pad)  # pstride = P + 7, NaN behind every row
    mu_v, _ = off(mean.cuda())
    al_v, _ = off(alpha.cuda())
    gz_v, _ = off(g_z.cuda())
    gl_v, _ = off(g_sld.cuda())
    go_v, go_buf = off(torch.zeros_like(go))
    gp_v, gp_buf = off(torch.zeros_like(gp), cols=P + pad)
    gp_buf[:] = float("nan")  # gradient rows need no initialisation; columns beyond P are not touched
    with launches(0, 1):
        assert lib.tnf_ctx_wide_sample_bwd_f32(z_v.data_ptr(), p_v.data_ptr(), mu_v.data_ptr(), al_v.data_ptr(),
                                               gz_v.data_ptr(), gl_v.data_ptr(), gp_v.data_ptr(), go_v.data_ptr(), M, N, D,
                                               S, L, U, P + pad, P + pad, L_.stream_ptr()) == 0
    assert torch.equal(go_v, go) and guards_intact(go_buf, go_v)
    assert torch.equal(gp_v, gp) and guards_intact(gp_buf, gp_v, cols=P + pad)


def test_closed_launch_gate_leaves_the_outputs_untouched(cws, oracle):
    D, S, L, U, M, N = 5, 2, 2, 20, 3, 9
    params, mean, alpha, omega = inputs(oracle, D, S, L, U, M, N)
    g_z, g_sld = R.upstream(M, N, D)
    oc, pc, mu, al, gz, gl = dev(omega, params, mean, alpha, g_z, g_sld)
    z = cws.ctx_wide_sample_train(oc, pc, mu, al, D, S, L, U)[0]
    P, st = params.shape[1], L_.stream_ptr()
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in ((M, P), (M, N, D))]

    def call():
        assert lib.tnf_ctx_wide_sample_bwd_f32(z.data_ptr(), pc.data_ptr(), mu.data_ptr(), al.data_ptr(), gz.data_ptr(),
                                               gl.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), M, N, D, S, L, U, P, P,
                                               st) == 0

    assert lib.tnf_set_launch_gate(gate.data_ptr()) == 0
    try:
        with launches(0, 1):  # the call reaches its launch; the kernel returns at once
            call()
        assert all(bool((o == 7.0).all()) for o in outs)
        gate.fill_(1)
        call()
        torch.cuda.synchronize()
    finally:
        assert lib.tnf_set_launch_gate(None) == 0
    gp, go = cws.ctx_wide_sample_bwd_raw(z, pc, mu, al, gz, gl, D, S, L, U)
    assert torch.equal(outs[0], gp) and torch.equal(outs[1], go)


def test_no_samples_no_launch(cws, oracle):
    D, S, L, U, M = 5, 2, 2, 20, 3
    params, mean, alpha, _ = inputs(oracle, D, S, L, U, M, 8)
    with launches(0, 0):
        gp, go = cws.ctx_wide_sample_bwd_raw(torch.zeros(M, 0, D).cuda(), params.cuda(), mean.cuda(), alpha.cuda(),
                                             torch.zeros(M, 0, D).cuda(), torch.zeros(M, 0).cuda(), D, S, L, U)
    assert gp.shape == params.shape and not gp.any() and go.shape == (M, 0, D)


# ---- through NormFlow and ConditionalDensityEstimator ---------------------------------------------------------------
def test_through_normflow_and_other_routes(tnf, cws, oracle):
    """Switch on: one forward launch, one backward launch, no diag family.  Switch off, N = 32 or no_grad: neither counter
    moves; with the switch off the gradients are within the bars of the same reference."""
    D, S, L, U, M = 5, 2, 2, 20, 5
    nf, params, mean, alpha, _ = CF.make_nf(tnf, oracle, D, S, L, U, M, 32)
    nf.context_rows = False
    omega = inputs(oracle, D, S, L, U, M, 32)[3]
    g_z, g_sld = R.upstream(M, 32, D)

    def nf_step(om, gz, gl):
        pc = params.cuda().requires_grad_()
        z, log_q = nf._forward_from(om.cuda(), pc, True)
        torch.autograd.backward([z, log_q], [gz.cuda(), -gl.double().cuda()])  # log_q = log N(omega) - sld
        return z.detach(), log_q.detach(), pc.grad

    def switched(value, fn):
        nf.wide_context_sample_training = value
        try:
            return fn()
        finally:
            nf.wide_context_sample_training = False

    o8, gz8, gl8 = omega[:, :8].contiguous(), g_z[:, :8].contiguous(), g_sld[:, :8].contiguous()
    with launches(1, 1):
        z_on, lq_on, gp_on = switched(True, lambda: nf_step(o8, gz8, gl8))
    want = R.reference(oracle, float64, o8, params, mean, alpha, gz8, gl8, (D, S, L, U))
    check("NormFlow, switch on", gp_on, None, want)
    before = counters()
    z_off, lq_off, gp_off = nf_step(o8, gz8, gl8)
    assert counters() == before
    check("NormFlow, switch off", gp_off, None, want)
    torch.testing.assert_close(z_on, z_off, **H.ZF_TOL)
    torch.testing.assert_close(lq_on, lq_off, **H.LQ_TOL)
    grad_err("ctx_wide_sample vs today's route params", gp_on, gp_off, BAR_P)
    nf.wide_context_rows = True  # the inference route's z and log_q, bit for bit
    with torch.no_grad():
        z_i, lq_i = nf._forward_from(o8.cuda(), params.cuda(), True)
    nf.wide_context_rows = False
    assert torch.equal(z_on, z_i) and torch.equal(lq_on, lq_i)
    before = counters()
    on, off = switched(True, lambda: nf_step(omega, g_z, g_sld)), nf_step(omega, g_z, g_sld)  # N = 32
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    with torch.no_grad():
        on = switched(True, lambda: nf._forward_from(o8.cuda(), params.cuda().requires_grad_(), True))
        off = nf._forward_from(o8.cuda(), params.cuda().requires_grad_(), True)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert counters() == before


def _cde(tnf, D, S, U, H_, seed, support=None):
    """domain_helpers._cde with an optional support layer; with one, the last Affine's log-scales are lowered by 2.5 so
    that the core's samples stay inside the range where a float32 ToInterval resolves its tanh (as in
    tests/test_gpu_ctx_sample.py)."""
    torch.manual_seed(seed)
    nf = tnf.NormFlow(D, True, "coupling", S, 2, U, support_layer=support)
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


@pytest.mark.parametrize("D,S,U,N,sup", [(4, 1, 20, 1, False), (4, 1, 20, 8, False), (5, 2, 64, 8, False), (4, 1, 20, 8, True)],
                         ids=["reference-cde-N=1", "U=20", "U=64", "U=20,ToInterval"])
def test_through_the_estimator(tnf, cws, oracle, D, S, U, N, sup):
    """z, log_q = cde(x, N, freeze_bn=True); loss = sum z^2 + sum log_q: one forward and one backward launch of the flow;
    param_net's gradients against the same call with the switch off and against float64 autograd through the float64 copy
    of the net and the oracle.  NormFlow(4, True, 'coupling', 1, 2, 20) is the reference's own conditional flow.  With a
    ToInterval support layer the core route is the same and the layer runs behind it as its own kernel."""
    M = 6
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    nf, cde = _cde(tnf, D, S, U, 32, seed=D + U + N, support=tnf.ToInterval(D, lb, ub) if sup else None)
    x = torch.randn(M, 8, generator=torch.Generator().manual_seed(D + U))

    def grads():
        cde.param_net.zero_grad(set_to_none=True)
        np.random.seed(17)
        z, log_q = cde(x.cuda(), N, freeze_bn=True)
        ((z ** 2).sum() + log_q.sum()).backward()
        return z.detach(), [p.grad.clone() for p in cde.param_net.parameters()]

    before = counters()
    z_off, off = grads()
    assert counters() == before
    nf.wide_context_sample_training = True
    with launches(1, 1):
        z_on, on = grads()
    np.random.seed(17)
    omega = np.random.normal(0.0, 1.0, (M, N, D))  # the draw cde made
    net64 = H._net64(cde)
    with float64():
        z64, lq64, _ = oracle.flow_forward(omega, net64(x.double()), D, S, 2, U, bn_stats=H._stats64_of(nf))
        if sup:
            z64, ld = oracle.to_interval(z64, tuple(c.double() for c in oracle.interval_consts(lb, ub)), False)
            lq64 = lq64 - ld
        ((z64 ** 2).sum() + lq64.sum()).backward()
    torch.testing.assert_close(z_on.cpu().double(), z64.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(z_on, z_off, rtol=1e-4, atol=1e-4)
    for i, (a, b, w) in enumerate(zip(on, off, net64.parameters())):
        tag = "ctx_wide_sample cde U=%d N=%d sup=%s p%d" % (U, N, sup, i)
        e_today, e_ref = grad_err(tag + " vs today", a, b), grad_err(tag + " vs float64", a, w.grad)
        print("%s: vs today's route %.3e, vs float64 %.3e" % (tag, e_today, e_ref))
        assert e_today <= BAR_P and e_ref <= BAR_P


def test_graph_capture(tnf, cws, oracle):
    """A whole step -- sampling forward, backward, into preallocated .grad -- captured on a single stream (no parallel
    branches) replays to the eager step's bits; the counters do not move on replay."""
    D, S, L, U, M, N = 6, 2, 2, 20, 7, 8
    nf, params, mean, alpha, omega = CF.make_nf(tnf, oracle, D, S, L, U, M, N)
    nf.context_rows = False
    nf.wide_context_sample_training = True
    g_z, g_sld = R.upstream(M, N, D)
    gz, gl = g_z.cuda(), -g_sld.double().cuda()
    pc, oc = params.cuda().requires_grad_(), omega.cuda()
    pc.grad = torch.zeros_like(pc)

    def one_step():
        pc.grad.zero_()
        z, log_q = nf._forward_from(oc, pc, True)
        torch.autograd.backward([z, log_q], [gz, gl])
        return z.detach(), log_q.detach()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the side stream
            one_step()
    torch.cuda.current_stream().wait_stream(s)
    with launches(1, 1):
        z_e, lq_e = one_step()
    z_eager, lq_eager, gp_eager = z_e.clone(), lq_e.clone(), pc.grad.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z, log_q = one_step()
    before = counters()
    pc.grad.fill_(7.0)
    z.zero_()
    log_q.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert counters() == before  # a replay runs the captured kernels; no call reaches the host launchers
    assert torch.equal(z, z_eager) and torch.equal(log_q, lq_eager) and torch.equal(pc.grad, gp_eager)
