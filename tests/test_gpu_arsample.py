"""Training an autoregressive flow through its samples in ONE backward kernel (csrc/maf_sample_bwd.hip,
include/tnf_arsample.h) against float64 autograd through the oracle: the bijector (`MAF.fused_sampling_backward`) and
the flow (`NormFlow.ar_sample_training`, family `ar_train_sample`).

Every gradient error is max |got - want| / max |want| (conftest.grad_err), measured for the new route AND for the
switch-off route (the code of before: tnf_maf_inverse_alpha, D + 1 tnf_maf_backward launches, ~3 D elementwise ops) on
the same inputs.  The bar of a shape is 4 x the switch-off route's error on that shape (README), and
never looser than what test_maf_sampling_direction_backward allows: 2e-4 of the largest entry.  The recorded errors are
in profiles/r17_arsample_grad_errors.json."""
import functools

import numpy as np
import pytest
import torch

from conftest import grad_err

pytestmark = pytest.mark.gpu

# (D, L, U, M, M_p, N): the smallest shapes at which each mechanism can fail
SHAPES = [
    (6, 2, 15, 3, 3, 40),      # per-context rows, plain-store flush, non-VEC loads, tail tile of 8 rows
    (5, 1, 20, 2, 1, 33),      # shared row, atomic flush, UT = 2, no hidden-to-hidden layer, tail of 1
    (16, 2, 32, 2, 2, 50),     # VEC loads, UT = 2
    (32, 3, 16, 1, 1, 40),     # DT = 2, L at its maximum
    (21, 2, 42, 2, 2, 100),    # the LFI shape: shared accumulator copy (nacc = 1), seven tiles over four waves
    (2, 1, 15, 1, 1, 1),       # one sweep, 15 padded rows that must add nothing
    (4, 2, 15, 1, 1, 40000),   # more tiles than a full grid's waves
]
CAP = 2e-4  # test_maf_sampling_direction_backward: atol 2e-4 max |g| (its rtol 2e-3 only loosens that)


def bar_of(err_off):
    return min(4.0 * err_off, CAP)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available()
    return torch_nf_amd


def counts(tnf):
    from torch_nf_amd import _lib, arsample_ops

    return arsample_ops.arsample_launch_count(), int(_lib.lib.tnf_diag_launch_count(_lib.DIAG_MAF_BWD_MFMA))


@functools.lru_cache(maxsize=None)
def problem(shape):
    """Inputs and the float64 references of one shape, computed once: the MAF's masks, parameters, base draw, loss
    weights, frozen statistics; d/d params and d/d omega at MAF level; d/d params of the three flow losses."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import flow_oracle as oracle
    import torch_nf_amd as tnf

    D, L, U, M, Mp, N = shape
    rng = np.random.RandomState(1000 * D + 10 * L + U)
    np.random.seed(D + L)
    maf = tnf.MAF(D, L, U)
    ms = [np.array(m) for m in maf.ms]
    Ms = [Mk[0].numpy().astype(np.float64) for Mk in maf.Ms]
    n = maf.count_num_params()
    pr = dict(ms=ms, n=n,
              p_maf=torch.tensor(rng.normal(0, 0.3, (Mp, n))),
              p_aff=torch.tensor(rng.normal(0, 0.2, (Mp, 2 * D))),
              omega=rng.normal(0, 1, (M, N, D)),
              wz=torch.tensor(rng.normal(0, 1, (M, N, D))), wl=torch.tensor(rng.normal(0, 1, (M, N))),
              mean=torch.tensor(rng.normal(0, 0.3, (D,))), alpha=torch.tensor(rng.uniform(0.5, 1.5, (D,))))
    # MAF level
    p, om = pr["p_maf"].clone().requires_grad_(), torch.tensor(pr["omega"]).requires_grad_()
    x, ld = oracle.maf(om, p, D, L, U, Ms, False)
    ((x * pr["wz"]).sum() + (ld * pr["wl"]).sum()).backward()
    pr["maf_gp"], pr["maf_gom"] = p.grad, om.grad
    # flow level: [MAF, BatchNorm (frozen), Affine] in float64, log_q = base - sum of log-dets
    pf = torch.cat([pr["p_maf"], pr["p_aff"]], 1)
    pr["p_flow"] = pf
    base = torch.tensor(oracle.base_log_density_f64(pr["omega"]))
    for name, cz, cl in (("both", 1.0, 1.0), ("z", 1.0, 0.0), ("log_q", 0.0, 1.0)):
        q = pf.clone().requires_grad_()
        x, ld = oracle.maf(torch.tensor(pr["omega"]), q[:, :n], D, L, U, Ms, False)
        y, ld2 = oracle.bn_forward_frozen(x, pr["mean"], pr["alpha"])
        z, ld3 = oracle.affine(y, q[:, n:], D, False)
        lq = base - ld - ld2 - ld3
        (cz * (z * pr["wz"]).sum() + cl * (lq * pr["wl"]).sum()).backward()
        pr["flow_gp_" + name] = q.grad
    return pr


def make_maf(tnf, shape, pr, fused):
    D, L, U = shape[:3]
    np.random.seed(0)
    maf = tnf.MAF(D, L, U)
    maf.set_masks(pr["ms"])
    maf.fused_sampling_backward = fused
    return maf


def make_flow(tnf, shape, pr, on, support=None):
    D, L, U = shape[:3]
    np.random.seed(0)
    nf = tnf.NormFlow(D, True, "AR", 1, L, U, support_layer=support)
    nf.bijectors[0].set_masks(pr["ms"])
    nf.bijectors[1].set_last_stats(pr["mean"].float().cuda(), pr["alpha"].float().cuda())
    nf.ar_sample_training = on
    return nf


def maf_grads(tnf, shape, pr, fused):
    maf = make_maf(tnf, shape, pr, fused)
    p = pr["p_maf"].float().cuda().requires_grad_()
    om = torch.tensor(pr["omega"]).float().cuda().requires_grad_()
    x, ld = maf(om, p)
    ((x * pr["wz"].float().cuda()).sum() + (ld * pr["wl"].float().cuda()).sum()).backward()
    return p.grad, om.grad, x.detach(), ld.detach()


def flow_grads(tnf, shape, pr, on, cz, cl):
    nf = make_flow(tnf, shape, pr, on)
    p = pr["p_flow"].float().cuda().requires_grad_()
    z, lq = nf._forward_from(pr["omega"], p, freeze_bn=True)
    (cz * (z * pr["wz"].float().cuda()).sum() + cl * (lq * pr["wl"].cuda()).sum()).backward()
    return p.grad, z.detach(), lq.detach()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d_L%d_U%d_M%d_Mp%d_N%d" % s)
def test_bijector_gradients(tnf, shape):
    """MAF.fused_sampling_backward = True: d/d params and d/d omega of sum(x w_z) + sum(ld w_l); forward values
    bit-identical; one launch of the new kernel and none of the inverse-direction backward."""
    pr = problem(shape)
    D = shape[0]
    c0 = counts(tnf)
    gp_off, gom_off, x_off, ld_off = maf_grads(tnf, shape, pr, False)
    c1 = counts(tnf)
    gp_on, gom_on, x_on, ld_on = maf_grads(tnf, shape, pr, True)
    c2 = counts(tnf)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, D + 1)
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 0)
    assert torch.equal(x_on, x_off) and torch.equal(ld_on, ld_off)
    tag = "arsample maf %s " % (shape,)
    for what, on, off, want in (("g_params", gp_on, gp_off, pr["maf_gp"]), ("g_omega", gom_on, gom_off, pr["maf_gom"])):
        e_off = grad_err(tag + what + " switch off", off, want)
        e_on = grad_err(tag + what, on, want)
        print(tag + what, "on %.3e off %.3e" % (e_on, e_off))
        grad_err(tag + what, on, want, bar_of(e_off))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d_L%d_U%d_M%d_Mp%d_N%d" % s)
def test_flow_gradients(tnf, shape):
    """NormFlow.ar_sample_training = True, frozen statistics: the route is ar_train_sample, z and log_q are those of
    the inference route bit for bit, and d/d params of sum(z w_z) + sum(log_q w_l) and of each term alone holds the bar."""
    pr = problem(shape)
    D = shape[0]
    nf = make_flow(tnf, shape, pr, True)
    p = pr["p_flow"].float().cuda().requires_grad_()
    assert nf._route("forward", torch.tensor(pr["omega"]).float().cuda(), p) == ("ar_train_sample", False, False)
    with torch.no_grad():
        z_inf, lq_inf = nf._forward_from(pr["omega"], p, freeze_bn=True)
    for name, cz, cl in (("both", 1.0, 1.0), ("z", 1.0, 0.0), ("log_q", 0.0, 1.0)):
        c0 = counts(tnf)
        g_off, _, _ = flow_grads(tnf, shape, pr, False, cz, cl)
        c1 = counts(tnf)
        g_on, z_on, lq_on = flow_grads(tnf, shape, pr, True, cz, cl)
        c2 = counts(tnf)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (0, D + 1)
        assert (c2[0] - c1[0], c2[1] - c1[1]) == (1, 0)
        assert torch.equal(z_on, z_inf) and torch.equal(lq_on, lq_inf)
        want = pr["flow_gp_" + name]
        tag = "arsample flow %s loss %s" % (shape, name)
        e_off = grad_err(tag + " switch off", g_off, want)
        e_on = grad_err(tag, g_on, want)
        print(tag, "on %.3e off %.3e" % (e_on, e_off))
        grad_err(tag, g_on, want, bar_of(e_off))


def test_per_context_rows_are_bit_reproducible(tnf):
    """Per-context rows with private accumulator copies: each gradient is written once, in a fixed order."""
    shape = SHAPES[0]
    pr = problem(shape)
    a = flow_grads(tnf, shape, pr, True, 1.0, 1.0)[0]
    b = flow_grads(tnf, shape, pr, True, 1.0, 1.0)[0]
    assert torch.equal(a, b)
    a = maf_grads(tnf, shape, pr, True)[0]
    b = maf_grads(tnf, shape, pr, True)[0]
    assert torch.equal(a, b)


def test_fresh_statistics(tnf, oracle):
    """freeze_bn=False with the switch on: the per-bijector composition, its MAF with the one-kernel sampling backward
    (shape and tolerance of test_ar_flow_sampling_with_gradients)."""
    D, L, U, M, N = 6, 2, 15, 2, 300
    np.random.seed(11)
    rng = np.random.RandomState(11)
    nf = tnf.NormFlow(D, True, "AR", 1, L, U)
    nf.ar_sample_training = True
    Ms = [Mk[0].numpy() for Mk in nf.bijectors[0].Ms]
    p0 = torch.tensor(rng.normal(0, 0.2, (M, nf.D_params))).float()
    omega = rng.normal(0, 1, (M, N, D))
    p = p0.clone().cuda().requires_grad_()
    c0 = counts(tnf)
    z, lq = nf._forward_from(omega, p, freeze_bn=False)
    loss = lq.mean() + (z ** 2).mean()
    loss.backward()
    c1 = counts(tnf)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0)
    assert nf.bijectors[0].fused_sampling_backward is False  # the switch held for the call only
    pr = p0.clone().requires_grad_()
    zr, lqr, _ = oracle.ar_flow_forward(omega, pr, D, nf.num_layers, nf.num_units, Ms, None)
    loss_r = lqr.mean() + (zr ** 2).mean()
    loss_r.backward()
    torch.testing.assert_close(loss.detach().cpu().double(), loss_r.detach().double(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(p.grad.cpu(), pr.grad, rtol=5e-3, atol=2e-4 * float(pr.grad.abs().max()))


def test_support_layer_behind_the_family(tnf):
    """A ToInterval support layer: the route is ar_train_sample with the layer as its own autograd op behind it; the
    gradient against the switch-off route's (the fused-free composition) error to float64 is not available without a
    float64 ToInterval here, so the two float32 routes are compared at the cap."""
    shape = SHAPES[0]
    D = shape[0]
    pr = problem(shape)
    lb, ub = -np.ones(D), np.ones(D) * 2
    grads = {}
    for on in (False, True):
        nf = make_flow(tnf, shape, pr, on, support=tnf.ToInterval(D, lb, ub))
        p = pr["p_flow"].float().cuda().requires_grad_()
        if on:
            assert nf._route("forward", torch.tensor(pr["omega"]).float().cuda(), p) == ("ar_train_sample", False, False)
        c0 = counts(tnf)
        z, lq = nf._forward_from(pr["omega"], p, freeze_bn=True)
        ((z * pr["wz"].float().cuda()).sum() + (lq * pr["wl"].cuda()).sum()).backward()
        c1 = counts(tnf)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if on else (0, D + 1))
        grads[on] = p.grad
    print("arsample ToInterval", "%.3e" % grad_err("arsample ToInterval on vs off", grads[True], grads[False]))
    grad_err("arsample ToInterval on vs off", grads[True], grads[False], CAP)


def test_through_the_conditional_density_estimator(tnf):
    """cde(x, N = 8, freeze_bn=True) with an AR estimator at D = 6: gradients reach every param_net parameter, equal to
    the switch-off route's within the cap."""
    D, L, U, M, N, Dx = 6, 2, 15, 4, 8, 3
    torch.manual_seed(5)
    np.random.seed(5)
    nf = tnf.NormFlow(D, True, "AR", 1, L, U)
    cde = tnf.ConditionalDensityEstimator(nf, Dx, [16])
    g = torch.Generator().manual_seed(6)
    nf.bijectors[1].set_last_stats(torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5)
    with torch.no_grad():
        for q in cde.param_net.parameters():
            q.mul_(0.5)
    cde.cuda()
    x = torch.randn(M, Dx, generator=g)
    wz, wl = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
    grads = {}
    for on in (False, True):
        nf.ar_sample_training = on
        cde.param_net.zero_grad()
        np.random.seed(11)
        c0 = counts(tnf)
        z, log_q = cde(x.cuda(), N=N, freeze_bn=True)
        ((z * wz.cuda()).sum() + (log_q * wl.cuda()).sum()).backward()
        c1 = counts(tnf)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if on else (0, D + 1))
        grads[on] = [q.grad.clone() for q in cde.param_net.parameters()]
    for (name, q), a, b in zip(cde.param_net.named_parameters(), grads[True], grads[False]):
        assert float(a.abs().max()) > 0
        tag = "arsample through the CDE: d " + name
        print(tag, "%.3e" % grad_err(tag, a, b))
        grad_err(tag, a, b, CAP)


def test_graph_capture_and_replay(tnf):
    """One torch.cuda.graph capture of sample -> loss -> backward (no parallel branches): the replay reproduces the
    eager gradient.  Per-context rows: bit-reproducible, so the bar is the eager route's own."""
    shape = SHAPES[0]
    pr = problem(shape)
    nf = make_flow(tnf, shape, pr, True)
    p = pr["p_flow"].float().cuda().requires_grad_()
    omega = torch.tensor(pr["omega"]).float().cuda()
    wz, wl = pr["wz"].float().cuda(), pr["wl"].cuda()

    def step():
        z, lq = nf._forward_from(omega, p, freeze_bn=True)
        return torch.autograd.grad((z * wz).sum() + (lq * wl).sum(), p)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step().clone()  # warm-up on the capture stream: workspaces and masks are allocated here
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = pr["flow_gp_both"]
    e_eager = grad_err("arsample graph eager", eager, want)
    print("arsample graph", "%.3e" % grad_err("arsample graph replay", out, want), "eager %.3e" % e_eager)
    grad_err("arsample graph replay", out, want, bar_of(e_eager))
