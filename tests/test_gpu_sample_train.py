"""Training through frozen-statistics sampling in one backward kernel (include/tnf_sampletrain.h,
NormFlow.sample_training) on the GPU: the route's parameter gradient against float64 autograd over oracle.flow_forward
at the bar the project holds the reversible log_prob pair to (BAR_P of tests/test_gpu_grad.py: the same split-f16
contractions and fixed-point sums); single cotangents; the values of the inference route bit for bit; the rebuilt base
draw against the existing inverse route; loss scales; reproducibility; launch accounting; overflow recovery; a support
layer; the conditional estimator; graph capture."""
import contextlib
import copy

import numpy as np
import pytest
import torch

from conftest import grad_err
from domain_helpers import float64

from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
BAR_P = 5e-5  # tests/test_gpu_grad.py

# (D, S, L, U, M, M_p, N): the smallest shapes at which each mechanism can fail
FIRST = (64, 4, 2, 15, 1, 1, 300)        # a tail tile of 12 rows
SHAPES = [FIRST,
          (32, 2, 3, 16, 3, 3, 33),      # per-row parameters, a tail of 1, U without the spare unit
          (64, 1, 1, 15, 3, 1, 50),      # a shared row flattened to M N, a two-layer ring that wraps every tile, no hidden layer
          (32, 8, 2, 15, 1, 1, 40),      # S at the accumulators' LDS limit
          (64, 4, 2, 15, 1, 1, 1)]       # 15 padded rows of the tile must add nothing
FIVE = (5, 2, 2, 15, 1, 1, 37)
PADDED = [(D, 2, 2, 15, 1, 1, 37) for D in (2, 5, 31, 33, 63)] + [(5, 2, 2, 15, 2, 2, 32)]
BWD_FAMILIES = (L_.DIAG_BWD_LAYER_FP32, L_.DIAG_BWD_LAYER_F16, L_.DIAG_BWD_GENERIC, L_.DIAG_BWD_FLOW_REV, L_.DIAG_BWD_WIDE)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@contextlib.contextmanager
def recovery(tnf, mode):
    fn = tnf.sampletrain_ops._FlowSampleFn
    before = fn.overflow_recovery
    fn.overflow_recovery = mode
    try:
        yield fn
    finally:
        fn.overflow_recovery = before


def counts():
    torch.cuda.synchronize()
    return [lib.tnf_diag_launch_count(f) for f in range(L_.DIAG_FAMILIES)], lib.tnf_sampletrain_launch_count()


_PROBLEMS = {}


def problem(oracle, shape, seed=0):
    """Inputs (float32, on the host) and the float64 reference of one shape, computed once: omega, params, the
    statistics, the loss weights, and d loss / d params of loss = sum z w_z + sum log_q w_l for (w_z, w_l), (w_z, 0) and
    (0, w_l)."""
    key = (shape, seed)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    D, S, L, U, M, Mp, N = shape
    rng = np.random.RandomState(1000 * D + 10 * S + N + seed)
    P = lib.tnf_flow_num_params(D, S, L, U)
    pr = dict(params=torch.from_numpy(rng.normal(0.0, 0.2, (Mp, P)).astype(np.float32)),
              mean=torch.from_numpy(rng.normal(0.0, 0.3, (2 * S, D)).astype(np.float32)),
              alpha=torch.from_numpy(rng.uniform(0.5, 1.5, (2 * S, D)).astype(np.float32)),
              omega=torch.from_numpy(rng.normal(0.0, 1.0, (M, N, D)).astype(np.float32)),
              wz=torch.from_numpy(rng.normal(0.0, 1.0, (M, N, D)).astype(np.float32)),
              wl=torch.from_numpy(rng.normal(0.0, 1.0, (M, N)).astype(np.float32)))
    stats = [(m.double(), a.double()) for m, a in zip(pr["mean"], pr["alpha"])]
    with float64():
        p = pr["params"].double().requires_grad_()
        z, log_q, _ = oracle.flow_forward(pr["omega"].double().numpy(), p, D, S, L, U, bn_stats=stats)
        lz, ll = (z * pr["wz"].double()).sum(), (log_q * pr["wl"].double()).sum()
        pr["g_z"], = torch.autograd.grad(lz, p, retain_graph=True)
        pr["g_l"], = torch.autograd.grad(ll, p)
        pr["g_both"] = pr["g_z"] + pr["g_l"]
        pr["z64"], pr["log_q64"] = z.detach(), log_q.detach()
    _PROBLEMS[key] = pr
    return pr


def make_flow(tnf, shape, pr, switch=True, support=None):
    D, S, L, U = shape[:4]
    nf = tnf.NormFlow(D, True, "coupling", S, L, U, support_layer=support)
    for b, m, a in zip(nf._bn_layers(), pr["mean"], pr["alpha"]):
        b.set_last_stats(m.cuda(), a.cuda())
    nf.sample_training = switch
    return nf


def step(nf, pr, use_z=True, use_l=True, scale=1.0, omega=None):
    """One sample -> loss -> backward through nf._forward_from -> (z, log_q, d loss / d params)."""
    p = pr["params"].cuda().requires_grad_()
    z, log_q = nf._forward_from(pr["omega"].cuda() if omega is None else omega, p, freeze_bn=True)
    loss = 0.0
    if use_z:
        loss = loss + (z * pr["wz"].cuda()).sum()
    if use_l:
        loss = loss + (log_q * pr["wl"].cuda()).sum()
    (loss * scale).backward()
    return z.detach(), log_q.detach(), p.grad


def name_of(shape):
    return "sample_train D=%d S=%d L=%d U=%d M=%d Mp=%d N=%d" % shape


# ---- the gradient ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + PADDED, ids=name_of)
def test_gradient_against_the_float64_oracle(tnf, oracle, shape):
    pr = problem(oracle, shape)
    nf = make_flow(tnf, shape, pr)
    p = pr["params"].cuda().requires_grad_()
    assert nf._route("forward", pr["omega"].cuda(), p).family == "train_sample"
    z, log_q, g = step(nf, pr)
    # (the values are the inference kernels', checked in their own tests: a sanity check of the reference's inputs)
    torch.testing.assert_close(z.cpu().double(), pr["z64"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(log_q.cpu(), pr["log_q64"], rtol=1e-4, atol=1e-4)
    assert g.shape == pr["params"].shape
    print(name_of(shape), "%.3e" % grad_err(name_of(shape), g, pr["g_both"]))
    grad_err(name_of(shape), g, pr["g_both"], BAR_P)


def test_several_tiles_per_wave(tnf, oracle):
    """N = 50016 is 3126 tiles, more than the 256 x 12 waves of a full grid: every workgroup walks the layers twice and the
    image ring wraps from layer 0 back to layer 2S-1 between a wave's tiles.  The loss is the reparameterised objective's
    shape, a mean over the samples (cotangents of one size); with random-sign weights the gradient grows like sqrt(N)
    while the fixed-point quantum grows with the tiles per workgroup, which is measured in DESIGN.md 20, not held here."""
    D, S, L, U, N = 32, 2, 2, 15, 50016
    rng = np.random.RandomState(3)
    P = lib.tnf_flow_num_params(D, S, L, U)
    pr = dict(params=torch.tensor(rng.normal(0, 0.2, (1, P))).float(), mean=torch.tensor(rng.normal(0, 0.3, (2 * S, D))).float(),
              alpha=torch.tensor(rng.uniform(0.5, 1.5, (2 * S, D))).float())
    omega = torch.tensor(rng.normal(0, 1, (1, N, D))).float()
    with float64():
        p64 = pr["params"].double().requires_grad_()
        stats = [(m.double(), a.double()) for m, a in zip(pr["mean"], pr["alpha"])]
        z64, lq64, _ = oracle.flow_forward(omega.double().numpy(), p64, D, S, L, U, bn_stats=stats)
        (z64.square().mean() + lq64.mean()).backward()
    nf = make_flow(tnf, (D, S, L, U), pr)
    p = pr["params"].cuda().requires_grad_()
    before = counts()[1]
    z, log_q = nf._forward_from(omega.cuda(), p, freeze_bn=True)
    (z.square().mean() + log_q.mean()).backward()
    assert counts()[1] == before + 1
    tag = "sample_train D=32 S=2 N=50016, two tiles per wave, mean loss"
    print(tag, "%.3e" % grad_err(tag, p.grad, p64.grad))
    grad_err(tag, p.grad, p64.grad, BAR_P)


@pytest.mark.parametrize("shape", [FIRST, FIVE], ids=name_of)
@pytest.mark.parametrize("which", ["z", "log_q"])
def test_single_cotangents(tnf, oracle, shape, which):
    """A loss from z only (g_sld absent) and from log_q only (g_z absent)."""
    pr = problem(oracle, shape)
    nf = make_flow(tnf, shape, pr)
    _, _, g = step(nf, pr, use_z=which == "z", use_l=which == "log_q")
    tag = name_of(shape) + " only " + which
    print(tag, "%.3e" % grad_err(tag, g, pr["g_z" if which == "z" else "g_l"]))
    grad_err(tag, g, pr["g_z" if which == "z" else "g_l"], BAR_P)


@pytest.mark.parametrize("shape", [FIRST, FIVE, (32, 2, 3, 16, 3, 3, 33)], ids=name_of)
@pytest.mark.parametrize("draw", ["numpy64", "torch32"])
def test_same_values_as_inference(tnf, oracle, shape, draw):
    """z and log_q with the switch on are those of the no-autograd call on the same omega, bit for bit."""
    pr = problem(oracle, shape)
    nf = make_flow(tnf, shape, pr)
    omega = pr["omega"].cuda() if draw == "torch32" else pr["omega"].double().numpy()
    p = pr["params"].cuda().requires_grad_()
    z, log_q = nf._forward_from(omega, p, freeze_bn=True)
    assert z.requires_grad and log_q.requires_grad
    with torch.no_grad():
        z0, log_q0 = nf._forward_from(omega, p, freeze_bn=True)
    assert torch.equal(z.detach(), z0) and torch.equal(log_q.detach(), log_q0)


# ---- the rebuilt base draw -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [FIRST, FIVE, (32, 2, 3, 16, 3, 3, 33)], ids=name_of)
def test_omega_out_of_the_raw_call(tnf, oracle, shape):
    """omega_out against the draw, held to 4 x the error of the existing inverse route on the same z."""
    D, S, L, U, M, Mp, N = shape
    pr = problem(oracle, shape)
    nf = make_flow(tnf, shape, pr)
    omega, p = pr["omega"].cuda(), pr["params"].cuda()
    with torch.no_grad():
        z, _ = nf._forward_from(omega, p, freeze_bn=True)
        z0, _ = nf.inverse_and_log_det(z, p)
    mean, alpha = nf._bn_stats(torch.device("cuda"))
    before = counts()[1]
    gp, om = tnf.sampletrain_ops.flow_sample_bwd_raw(z.contiguous(), p, p.shape[1], mean, alpha, pr["wz"].cuda(),
                                                     pr["wl"].cuda(), D, S, L, U, tuple(p.shape), want_omega=True)
    assert counts()[1] == before + 1
    err, yard = float((om - omega).abs().max()), float((z0 - omega).abs().max())
    print(name_of(shape), "omega_out error %.3e, inverse route %.3e" % (err, yard))
    assert yard > 0 and err <= 4 * yard, (err, yard)
    # the raw call's gradient is that of loss = sum z w_z + sum sum_log_det w_l: log_q = base - sum_log_det
    grad_err(name_of(shape) + " raw", gp, pr["g_z"] - pr["g_l"], BAR_P)


# ---- scales, reproducibility, launches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-7, 1e-3, 30.0, 3e4])
def test_loss_scales(tnf, oracle, scale):
    """The power-of-two pre-scale makes the relative error independent of the loss scale."""
    pr = problem(oracle, FIRST)
    nf = make_flow(tnf, FIRST, pr)
    _, _, g = step(nf, pr, scale=scale)
    tag = name_of(FIRST) + " loss x %g" % scale
    print(tag, "%.3e" % grad_err(tag, g, pr["g_both"] * scale))
    grad_err(tag, g, pr["g_both"] * scale, BAR_P)


@pytest.mark.parametrize("shape", [FIRST, (5, 2, 2, 15, 2, 2, 32), (64, 1, 1, 15, 3, 1, 50)], ids=name_of)
def test_backward_is_reproducible_bit_for_bit(tnf, oracle, shape):
    pr = problem(oracle, shape)
    nf = make_flow(tnf, shape, pr)
    g1, g2 = step(nf, pr)[2], step(nf, pr)[2]
    assert bool(torch.isfinite(g1).all()) and torch.equal(g1, g2)


@pytest.mark.parametrize("shape", [FIRST, FIVE], ids=name_of)
def test_launch_accounting(tnf, oracle, shape):
    pr = problem(oracle, shape)
    for switch in (True, False):
        nf = make_flow(tnf, shape, pr, switch=switch)
        p = pr["params"].cuda().requires_grad_()
        z, log_q = nf._forward_from(pr["omega"].cuda(), p, freeze_bn=True)
        loss = (z * pr["wz"].cuda()).sum() + (log_q * pr["wl"].cuda()).sum()
        diag0, n0 = counts()
        loss.backward()
        diag1, n1 = counts()
        moved = [f for f in BWD_FAMILIES if diag1[f] != diag0[f]]
        if switch:  # one backward: exactly one call of the new entry, no per-bijector backward family
            assert n1 == n0 + 1 and not moved, (n1 - n0, moved)
        else:  # today's route: the composition's backward kernels, the new counter still
            assert n1 == n0 and moved, (n1 - n0, moved)


# ---- overflow ------------------------------------------------------------------------------------------------------------
def test_overflow_recovery(tnf, oracle):
    """The budget of the header is 2^13 per accumulated term in units where the largest cotangent is in [1, 2).  A draw
    row k sigma out gives d_s = g2 (v2 - t) of about k times the row's cotangent; with loss weights of one size (all
    cotangents in [1, 2) after the pre-scale) k = 3e4 > 2^13 exceeds it -- asserted through overflow_fallbacks.  "host"
    then gives the gradient of the per-bijector composition, within the tolerances of
    tests/test_gpu_grad.py::test_flow_reversible_backward_overflow_falls_back; "off" gives NaN; a clean draw leaves the
    flag at 0 and both modes give identical bits."""
    shape = (64, 4, 2, 15, 1, 1, 512)
    D, S, L, U, M, Mp, N = shape
    rng = np.random.RandomState(1)
    P = lib.tnf_flow_num_params(D, S, L, U)
    pr = dict(params=torch.tensor(rng.normal(0, 0.05, (1, P))).float(), mean=torch.zeros(2 * S, D), alpha=torch.ones(2 * S, D),
              wz=torch.tensor(rng.choice([-1.0, 1.0], (1, N, D))).float(), wl=torch.tensor(rng.choice([-1.0, 1.0], (1, N))).float())
    clean = torch.tensor(rng.normal(0, 1, (1, N, D))).float()
    bad = clean.clone()
    bad[0, ::128] *= 3e4
    with float64():
        p_ref = pr["params"].double().requires_grad_()
        stats = [(m.double(), a.double()) for m, a in zip(pr["mean"], pr["alpha"])]
        z, log_q, _ = oracle.flow_forward(bad.double().numpy(), p_ref, D, S, L, U, bn_stats=stats)
        ((z * pr["wz"].double()).sum() + (log_q * pr["wl"].double()).sum()).backward()
    scale = float(p_ref.grad.abs().max())
    nf = make_flow(tnf, shape, pr)
    with recovery(tnf, "host") as fn:
        before = fn.overflow_fallbacks
        _, _, g = step(nf, pr, omega=bad.cuda())
        assert fn.overflow_fallbacks == before + 1, "the fixed-point budget must have been exceeded by this input"
        assert int(fn.last_overflow_flag.item()) == 1
        assert bool(torch.isfinite(g).all())
        torch.testing.assert_close(g.cpu().double() / scale, p_ref.grad / scale, rtol=2e-3, atol=2e-5)
    with recovery(tnf, "off"):
        _, _, g = step(nf, pr, omega=bad.cuda())
        assert bool(torch.isnan(g).any())
    grads = []
    for mode in ("host", "off"):
        with recovery(tnf, mode) as fn:
            before = fn.overflow_fallbacks
            grads.append(step(nf, pr, omega=clean.cuda())[2])
            assert fn.overflow_fallbacks == before
            if mode == "host":
                assert int(fn.last_overflow_flag.item()) == 0
    assert bool(torch.isfinite(grads[0]).all()) and torch.equal(grads[0], grads[1])


# ---- a support layer, the conditional estimator, a captured step ------------------------------------------------------------
def test_support_layer_runs_behind_the_family(tnf, oracle):
    """NormFlow(4, ..., support_layer=ToInterval): the route is train_sample, the support layer runs as its own autograd
    op behind it.  With the common statistics and parameters the core's samples reach |z| = 32, where float32 tanh is
    saturated (1 - tanh^2 < 2^-24 beyond |z| = 8.7) and no float32 ToInterval can be compared with float64; the last
    Affine's log-scales are lowered by 2.5 here, which keeps the core's samples within |z| < 3 (measured 2.9), inside the
    interval map's resolved range as a fitted flow's are."""
    shape = (4, 2, 2, 15, 1, 1, 37)
    D, S, L, U, M, Mp, N = shape
    pr = dict(problem(oracle, shape))
    pr["params"] = pr["params"].clone()
    pr["params"][:, -2 * D:-D] -= 2.5
    lb, ub = [-1.0, 0.0, -2.0, 1.0], [2.0, 3.0, 0.5, 4.0]
    nf = make_flow(tnf, shape, pr, support=tnf.ToInterval(D, lb, ub))
    p = pr["params"].cuda().requires_grad_()
    assert nf._route("forward", pr["omega"].cuda(), p) == ("train_sample", False, False)
    before = counts()[1]
    z, log_q, g = step(nf, pr)
    assert counts()[1] == before + 1
    with float64():
        p64 = pr["params"].double().requires_grad_()
        stats = [(m.double(), a.double()) for m, a in zip(pr["mean"], pr["alpha"])]
        zc, lq, _ = oracle.flow_forward(pr["omega"].double().numpy(), p64, D, S, L, U, bn_stats=stats)
        zs, ld = oracle.to_interval(zc, oracle.interval_consts(np.array(lb), np.array(ub)), False)
        lq = lq - ld
        ((zs * pr["wz"].double()).sum() + (lq * pr["wl"].double()).sum()).backward()
    assert bool((z.cpu() >= torch.tensor(lb)).all()) and bool((z.cpu() <= torch.tensor(ub)).all())  # (float32 saturates)
    torch.testing.assert_close(z.cpu().double(), zs.detach(), rtol=1e-4, atol=1e-4)
    print("support", "%.3e" % grad_err("sample_train ToInterval D=4", g, p64.grad))
    grad_err("sample_train ToInterval D=4", g, p64.grad, BAR_P)


def test_through_the_conditional_density_estimator(tnf, oracle):
    """cde(x, N = 32, freeze_bn=True) with 4 contexts at D = 64: the gradient of every param_net parameter against float64
    autograd through a .double() copy of param_net and the oracle."""
    D, S, L, U, M, N, Dx = 64, 2, 2, 15, 4, 32, 3
    torch.manual_seed(5)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    cde = tnf.ConditionalDensityEstimator(nf, Dx, [16])
    g = torch.Generator().manual_seed(6)
    for b in nf._bn_layers():
        b.set_last_stats(torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5)
    with torch.no_grad():
        for q in cde.param_net.parameters():
            q.mul_(0.5)
    net64 = copy.deepcopy(cde.param_net).cpu().double()
    cde.cuda()
    nf.sample_training = True
    x = torch.randn(M, Dx, generator=g)
    wz, wl = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
    np.random.seed(11)
    before = counts()[1]
    z, log_q = cde(x.cuda(), N=N, freeze_bn=True)
    ((z * wz.cuda()).sum() + (log_q * wl.cuda()).sum()).backward()
    assert counts()[1] == before + 1  # the route was train_sample
    np.random.seed(11)
    omega = np.random.normal(0.0, 1.0, (M, N, D))  # the draw cde made
    with float64():
        stats = [(b.get_last_mean().cpu().double(), b.get_last_alpha().cpu().double()) for b in nf._bn_layers()]
        z64, lq64, _ = oracle.flow_forward(omega, net64(x.double()), D, S, L, U, bn_stats=stats)
        ((z64 * wz.double()).sum() + (lq64 * wl.double()).sum()).backward()
    torch.testing.assert_close(z.detach().cpu().double(), z64.detach(), rtol=1e-4, atol=1e-4)
    for (name, q), q64 in zip(cde.param_net.named_parameters(), net64.parameters()):
        tag = "sample_train through the CDE: d " + name
        print(tag, "%.3e" % grad_err(tag, q.grad, q64.grad))
        grad_err(tag, q.grad, q64.grad, BAR_P)


def test_graph_captured_step_replays_the_eager_gradient(tnf, oracle):
    """sample -> loss -> backward with recovery "off", captured by graphs.GraphedStep: every launch of the route is
    capturable (no allocation inside the C call, no synchronisation), and the replay gives the eager gradient bit for bit."""
    from torch_nf_amd.graphs import GraphedStep

    for shape in (FIRST, FIVE):
        pr = problem(oracle, shape)
        nf = make_flow(tnf, shape, pr)
        omega, wz, wl = pr["omega"].cuda(), pr["wz"].cuda(), pr["wl"].cuda()
        with recovery(tnf, "off"):
            eager = step(nf, pr)[2]
            p = pr["params"].cuda().requires_grad_()
            grad_out = torch.zeros_like(p)

            def one():
                p.grad = None
                z, log_q = nf._forward_from(omega, p, freeze_bn=True)
                ((z * wz).sum() + (log_q * wl).sum()).backward()
                grad_out.copy_(p.grad)
                return grad_out

            before = counts()[1]
            gs = GraphedStep(one, warmup=2)
            g1 = gs().clone()
            g2 = gs().clone()
            torch.cuda.synchronize()
            assert counts()[1] > before
        assert bool(torch.isfinite(g1).all()) and torch.equal(g1, eager) and torch.equal(g2, eager)
