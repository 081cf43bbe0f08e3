"""Per-context coupling flows with fewer than 32 samples per context in one launch (include/tnf_ctxflow.h,
csrc/flow_ctx.hip, NormFlow's family `context_rows`) against the CPU oracle run in float64 on float64 copies of the same
float32 inputs, with per-context parameter rows.  Rows are xavier_normal_ (even contexts) and N(0, 0.1) (odd contexts),
the BatchNorm statistics come from one recorded oracle forward, z ~ N(0, 1).  Tolerances are the suite's own bars
(tests/domain_helpers.py): the same exact-f32 MFMA tile meets them per layer in tests/test_gpu_domain.py.  The launch
counters check that each call is ONE launch of the new kernel and nothing else."""
import numpy as np
import pytest
import torch

import domain_helpers as H
from domain_helpers import INV_TOL, LOGP_TOL, LQ_TOL, SLDF_TOL, ZF_TOL, float64
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
WG = 4  # contexts (waves) per workgroup of the kernel: ctxflow_ops.WAVES_PER_WORKGROUP


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def cx(tnf):
    from torch_nf_amd import ctxflow_ops

    assert ctxflow_ops.WAVES_PER_WORKGROUP == WG
    return ctxflow_ops


def ctx_counts():
    torch.cuda.synchronize()
    return [lib.tnf_ctx_flow_launch_count(0), lib.tnf_ctx_flow_launch_count(1)]


class one_launch(object):
    """`with one_launch(lp, fwd)`: the block moves the two new counters by exactly (lp, fwd) and no diag family."""

    def __init__(self, lp, fwd):
        self.want = [lp, fwd]

    def __enter__(self):
        self.ctx, self.diag = ctx_counts(), H.counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(ctx_counts(), self.ctx)] == self.want
            assert H.launched(self.diag) == {}
        return False


_INPUTS = {}


def inputs(oracle, D, S, L, U, M, N, seed=0, Mz=None):
    """(params (M, P), mean (2S, D), alpha (2S, D), z (Mz, N, D)) float32 on the host; computed once per case."""
    key = (D, S, L, U, M, N, seed, Mz)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * D + 10 * N + seed)
        P = oracle.flow_num_params(D, S, L, U)
        params = torch.randn(M, P, generator=g) * 0.1
        torch.manual_seed(1000 * D + seed)
        xav = torch.nn.init.xavier_normal_(torch.zeros(M, P))
        params[::2] = xav[::2]
        omega = torch.randn(M, 16, D, generator=g).double().numpy()
        _, _, stats = oracle.flow_forward(omega, params, D, S, L, U)  # one recorded forward: its batch statistics
        mean = torch.stack([m for m, _ in stats]).float().contiguous()
        alpha = torch.stack([a for _, a in stats]).float().contiguous()
        z = torch.randn(M if Mz is None else Mz, N, D, generator=g)
        _INPUTS[key] = (params, mean, alpha, z)
    return _INPUTS[key]


def st64(mean, alpha):
    return [(m.double(), a.double()) for m, a in zip(mean, alpha)]


def ref_inverse(oracle, z, params, mean, alpha, D, S, L, U):
    with float64():
        z0, sld = oracle.flow_inverse(z.double(), params.double(), D, S, L, U, st64(mean, alpha))
        lp = oracle.flow_log_prob(z.double(), params.double(), D, S, L, U, st64(mean, alpha))
    return lp, z0, sld.double()


def ref_forward(oracle, omega, params, mean, alpha, D, S, L, U):
    with float64():
        z, lq, _ = oracle.flow_forward(omega.double().numpy(), params.double(), D, S, L, U, st64(mean, alpha))
    sld = torch.from_numpy(oracle.base_log_density_f64(omega.double().numpy())) - lq
    return z, sld, lq


def check_inverse(got, want):
    lp, z0, sld = got
    torch.testing.assert_close(lp.cpu().double(), want[0], **LOGP_TOL)
    torch.testing.assert_close(z0.cpu().double(), want[1], **INV_TOL)
    torch.testing.assert_close(sld.cpu().double(), want[2], **INV_TOL)


def check_forward(got, want):
    z, sld, lq = got
    torch.testing.assert_close(z.cpu().double(), want[0], **ZF_TOL)
    torch.testing.assert_close(sld.cpu().double(), want[1], **SLDF_TOL)
    torch.testing.assert_close(lq.cpu().double(), want[2], **LQ_TOL)


def run_inverse(cx, z, params, mean, alpha, shape):
    return cx.ctx_flow_log_prob_raw(z.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), *shape, want_lp=True, want_z0=True,
                                    want_sld=True)


def run_forward(tnf, cx, omega, params, mean, alpha, shape):
    """(z, sum_log_det, log_q): the float64 log_q formed the way NormFlow forms it on this route."""
    oc = omega.cuda()
    z, sld = cx.ctx_flow_forward_raw(oc, params.cuda(), mean.cuda(), alpha.cuda(), *shape)
    return z, sld, tnf.ops.base_log_density_f64(oc) - sld


def both_directions(tnf, cx, oracle, D, S, L, U, M, N):
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    shape = (D, S, L, U)
    with one_launch(1, 0):
        got = run_inverse(cx, z, params, mean, alpha, shape)
    check_inverse(got, ref_inverse(oracle, z, params, mean, alpha, *shape))
    with one_launch(0, 1):
        z_f, sld_f = cx.ctx_flow_forward_raw(z.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), *shape)
    lq = tnf.ops.base_log_density_f64(z.cuda()) - sld_f
    check_forward((z_f, sld_f, lq), ref_forward(oracle, z, params, mean, alpha, *shape))


# ---- the domain, through the ops entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 31])
@pytest.mark.parametrize("D", [2, 5, 16, 31, 32, 33, 63, 64])
def test_widths_and_tiles(tnf, cx, oracle, D, N):
    """Both tile widths, both parities, the smallest and largest padding and none; one tile, the tile edge, a partial
    second tile; M = 5 is a partial last workgroup."""
    both_directions(tnf, cx, oracle, D, 2, 2, 15, 5, N)


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D", [5, 64])
def test_depth_and_units(tnf, cx, oracle, D, L, S):
    """num_units = 16 (no padded hidden unit), every depth of the template, and S = 9: beyond every LDS-image limit of
    the other whole-flow kernels."""
    both_directions(tnf, cx, oracle, D, S, L, 16, 3, 7)


@pytest.mark.parametrize("M", [1, WG - 1, WG, WG + 1])
def test_workgroup_edges(tnf, cx, oracle, M):
    both_directions(tnf, cx, oracle, 6, 2, 2, 15, M, 3)


def test_rows_stay_with_their_contexts(tnf, cx, oracle):
    """Context m's outputs are those of a call with that context alone, bit for bit, and a permutation of the contexts
    permutes the outputs."""
    D, S, L, U, M, N = 6, 2, 2, 15, 6, 5
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, seed=3)
    assert len({tuple(r.tolist()) for r in params}) == M  # pairwise different rows
    shape = (D, S, L, U)
    got = run_inverse(cx, z, params, mean, alpha, shape)
    fwd = run_forward(tnf, cx, z, params, mean, alpha, shape)
    for m in range(M):
        alone = run_inverse(cx, z[m:m + 1], params[m:m + 1], mean, alpha, shape)
        alone_f = run_forward(tnf, cx, z[m:m + 1], params[m:m + 1], mean, alpha, shape)
        for a, b in zip(got + fwd, alone + alone_f):
            assert torch.equal(a[m:m + 1], b), m
    perm = torch.tensor([4, 0, 5, 2, 1, 3])
    got_p = run_inverse(cx, z[perm], params[perm], mean, alpha, shape)
    fwd_p = run_forward(tnf, cx, z[perm], params[perm], mean, alpha, shape)
    for a, b in zip(got + fwd, got_p + fwd_p):
        assert torch.equal(a[perm.cuda()], b)


def test_one_block_of_z_for_every_context(tnf, cx, oracle):
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 9
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, Mz=1)
    assert z.shape[0] == 1
    with one_launch(1, 0):
        got = run_inverse(cx, z, params, mean, alpha, (D, S, L, U))
    assert got[0].shape == (M, N) and got[1].shape == (M, N, D)
    check_inverse(got, ref_inverse(oracle, z.expand(M, N, D), params, mean, alpha, D, S, L, U))


def test_longer_rows_and_expanded_views(tnf, cx, oracle):
    """A row stride beyond the row (trailing parameters are ignored, the view is not copied) and an expanded single row
    (stride 0: staged as M rows)."""
    D, S, L, U, M, N = 7, 2, 2, 15, 5, 4
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    shape = (D, S, L, U)
    P = params.shape[1]
    want = ref_inverse(oracle, z, params, mean, alpha, *shape)
    plain = run_inverse(cx, z, params, mean, alpha, shape)
    wide = torch.full((M, P + 7), float("nan"))
    wide[:, :P] = params
    with one_launch(1, 0):
        got = run_inverse(cx, z, wide, mean, alpha, shape)  # pstride = P + 7, the NaNs behind the row never read
    check_inverse(got, want)
    view = wide.cuda()[:, :P]
    assert view.stride(0) == P + 7 and not view.is_contiguous()
    got_v = cx.ctx_flow_log_prob_raw(z.cuda(), view, mean.cuda(), alpha.cuda(), *shape, want_lp=True, want_z0=True,
                                     want_sld=True)
    for a, b in zip(got_v, plain):
        assert torch.equal(a, b)
    row = params[1:2]
    expanded = row.cuda().expand(M, P)
    assert expanded.stride(0) == 0
    got_e = cx.ctx_flow_log_prob_raw(z.cuda(), expanded, mean.cuda(), alpha.cuda(), *shape, want_lp=True, want_z0=True,
                                     want_sld=True)
    check_inverse(got_e, ref_inverse(oracle, z, row.expand(M, P), mean, alpha, *shape))
    got_r = run_inverse(cx, z, row.repeat(M, 1), mean, alpha, shape)
    for a, b in zip(got_e, got_r):
        assert torch.equal(a, b)


def test_subsets_of_the_outputs(tnf, cx, oracle):
    D, S, L, U, M, N = 33, 1, 2, 15, 3, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    full = run_inverse(cx, z, params, mean, alpha, (D, S, L, U))
    dev = (z.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), D, S, L, U)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        got = cx.ctx_flow_log_prob_raw(*dev, want_lp=want[0], want_z0=want[1], want_sld=want[2])
        for w, a, b in zip(want, got, full):
            assert (a is None) if not w else torch.equal(a, b)


# ---- through NormFlow and ConditionalDensityEstimator ---------------------------------------------------------------
def make_nf(tnf, oracle, D, S, L, U, M, N, support=None, seed=0):
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, seed=seed)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U, support_layer=support)
    for b, m, a in zip(nf._bn_layers(), mean, alpha):
        b.set_last_stats(m.cuda(), a.cuda())
    nf.context_rows = True
    return nf, params, mean, alpha, z


def test_round_trip(tnf, oracle):
    D, S, L, U, M, N = 33, 2, 2, 15, 5, 11
    nf, params, mean, alpha, omega = make_nf(tnf, oracle, D, S, L, U, M, N)
    with torch.no_grad(), one_launch(1, 1):
        z, _ = nf._forward_from(omega.cuda(), params.cuda(), freeze_bn=True)
        back, _ = nf.inverse_and_log_det(z, params.cuda())
    torch.testing.assert_close(back.cpu(), omega, **INV_TOL)


@pytest.mark.parametrize("D", [4, 64])
def test_conditional_estimator_calls(tnf, oracle, D):
    """cde.log_prob(z (M, 8, D), x), cde(x, N = 8, freeze_bn=True) and cde.sample(x, 8): each is one launch of the new
    kernel and no other flow kernel, and agrees with the float64 oracle on the materialised parameter rows."""
    S, L, M, N = (1 if D == 4 else 4), 2, 6, 8
    nf, cde = H._cde(tnf, D, S, L, 100 if D == 4 else 32, seed=D)
    nf.context_rows = True
    g = torch.Generator().manual_seed(D)
    x = torch.randn(M, 8, generator=g)
    z = torch.randn(M, N, D, generator=g)
    with float64():
        params64 = H._net64(cde)(x.double()).detach()
    stats = H._stats64_of(nf)
    shape = (D, S, L, 15)
    with torch.no_grad():
        with one_launch(1, 0):
            lp = cde.log_prob(z.cuda(), x.cuda())
        with float64():
            want = oracle.flow_log_prob(z.double(), params64, *shape, stats)
        torch.testing.assert_close(lp.cpu().double(), want, **LOGP_TOL)

        np.random.seed(7)
        with one_launch(0, 1):
            zs, lq = cde(x.cuda(), N=N, freeze_bn=True)
        np.random.seed(7)
        omega = np.random.normal(0.0, 1.0, (M, N, D))
        with float64():
            z_w, lq_w, _ = oracle.flow_forward(omega, params64, *shape, stats)
        torch.testing.assert_close(zs.cpu().double(), z_w, **ZF_TOL)
        torch.testing.assert_close(lq.cpu(), lq_w, **LQ_TOL)

        gen = torch.Generator(device="cuda").manual_seed(11)
        with one_launch(0, 1):
            zs, lq = cde.sample(x.cuda(), N, generator=gen)
        gen.manual_seed(11)
        omega = torch.randn((M, N, D), device="cuda", dtype=torch.float32, generator=gen).cpu()
        with float64():
            z_w, lq_w, _ = oracle.flow_forward(omega.double().numpy(), params64, *shape, stats)
        torch.testing.assert_close(zs.cpu().double(), z_w, **ZF_TOL)
        torch.testing.assert_close(lq.cpu(), lq_w, **LQ_TOL)


def test_support_layer_runs_as_its_own_kernel(tnf, oracle):
    D, S, L, U, M, N = 5, 2, 2, 15, 5, 8
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    nf, params, mean, alpha, _ = make_nf(tnf, oracle, D, S, L, U, M, N, support=tnf.ToInterval(D, lb, ub))
    z = torch.from_numpy(np.random.RandomState(0).uniform(-1.5, 2.5, (M, N, D)).astype(np.float32))
    consts = tuple(c.double() for c in oracle.interval_consts(lb, ub))
    with torch.no_grad():
        before = ctx_counts()
        lp = nf.log_prob(z.cuda(), params.cuda())
        assert [a - b for a, b in zip(ctx_counts(), before)] == [1, 0]
        with float64():
            z_in, ld_sup = oracle.to_interval(z.double(), consts, True)
            want = oracle.flow_log_prob(z_in, params.double(), D, S, L, U, st64(mean, alpha)) - ld_sup
        torch.testing.assert_close(lp.cpu().double(), want, **LOGP_TOL)
        omega = torch.randn(M, N, D, generator=torch.Generator().manual_seed(4))
        before = ctx_counts()
        zs, lq = nf._forward_from(omega.double().numpy(), params.cuda(), freeze_bn=True)
        assert [a - b for a, b in zip(ctx_counts(), before)] == [0, 1]
        with float64():
            z_c, lq_c, _ = oracle.flow_forward(omega.double().numpy(), params.double(), D, S, L, U, st64(mean, alpha))
            z_w, ld = oracle.to_interval(z_c, consts, False)
        torch.testing.assert_close(zs.cpu().double(), z_w, **ZF_TOL)
        torch.testing.assert_close(lq.cpu(), lq_c - ld, **LQ_TOL)
        # inverse_and_log_det of a flow with a support layer stays on the bijectors
        before = ctx_counts()
        nf.inverse_and_log_det(z.cuda(), params.cuda())
        assert ctx_counts() == before


def test_other_calls_keep_their_routes(tnf, oracle):
    """Switch off, N = 32, or rows that require grad: the new counters do not move and the result is today's."""
    D, S, L, U, M = 5, 2, 2, 15, 5
    nf, params, mean, alpha, _ = make_nf(tnf, oracle, D, S, L, U, M, 32)
    z = inputs(oracle, D, S, L, U, M, 32)[3].cuda()
    pc = params.cuda()

    def today(fn):
        nf.context_rows = False
        try:
            return fn()
        finally:
            nf.context_rows = True

    before = ctx_counts()
    with torch.no_grad():
        off = today(lambda: nf.log_prob(z[:, :8], pc))
        assert ctx_counts() == before
        on = nf.log_prob(z[:, :8], pc)
        assert ctx_counts() == [before[0] + 1, before[1]]
        torch.testing.assert_close(on, off, **LOGP_TOL)
        before = ctx_counts()
        assert torch.equal(nf.log_prob(z, pc), today(lambda: nf.log_prob(z, pc)))  # N = 32
        zs, lq = nf._forward_from(np.zeros((M, 32, D)), pc, freeze_bn=True)
        zs_t, lq_t = today(lambda: nf._forward_from(np.zeros((M, 32, D)), pc, freeze_bn=True))
        assert torch.equal(zs, zs_t) and torch.equal(lq, lq_t)
    pg = pc.clone().requires_grad_()
    lp = nf.log_prob(z[:, :8], pg)
    lp_t = today(lambda: nf.log_prob(z[:, :8], pg))
    assert lp.requires_grad and torch.equal(lp, lp_t)
    assert ctx_counts() == before


def test_agrees_with_the_composition_at_d64(tnf, oracle):
    """D = 64 with the fused conditioner off: the new route against the route the same call takes with the switch off,
    on the same tensors."""
    D, S, L, M, N = 64, 4, 2, 9, 8
    nf, cde = H._cde(tnf, D, S, L, 32, seed=3)
    cde.fuse_conditioner = False
    g = torch.Generator().manual_seed(5)
    x, z = torch.randn(M, 8, generator=g).cuda(), torch.randn(M, N, D, generator=g).cuda()
    with torch.no_grad():
        before = ctx_counts()
        old = cde.log_prob(z, x)
        np.random.seed(3)
        zs_old, lq_old = cde(x, N=N, freeze_bn=True)
        assert ctx_counts() == before
        nf.context_rows = True
        new = cde.log_prob(z, x)
        np.random.seed(3)
        zs_new, lq_new = cde(x, N=N, freeze_bn=True)
        assert ctx_counts() == [before[0] + 1, before[1] + 1]
    torch.testing.assert_close(new, old, **LOGP_TOL)
    torch.testing.assert_close(zs_new, zs_old, **ZF_TOL)
    torch.testing.assert_close(lq_new, lq_old, **LQ_TOL)


def test_graph_capture(tnf, cx, oracle):
    """One log_prob call captured on a single stream (no parallel branches) replays to the same bits."""
    D, S, L, U, M, N = 6, 2, 2, 15, 7, 8
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    dev = (params.cuda(), mean.cuda(), alpha.cuda())
    zc = z.cuda()
    eager = cx.ctx_flow_log_prob_raw(zc, *dev, D, S, L, U)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cx.ctx_flow_log_prob_raw(zc, *dev, D, S, L, U)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lp = cx.ctx_flow_log_prob_raw(zc, *dev, D, S, L, U)[0]
    before = ctx_counts()
    lp.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert ctx_counts() == before  # a replay runs the captured kernel; no call reaches the host launcher
    assert torch.equal(lp, eager)
