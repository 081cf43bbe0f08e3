"""Training coupling flows of width 2 <= D <= 63 through the one-kernel reversible backward at the embedded width 2H
(include/tnf_padtrain.h, NormFlow.padded_training) on the GPU: the four layout kernels against torch indexing with the
restated map of tests/test_padded_train_host.py; the route's gradients bit for bit against the existing reversible pair
run at width 2H on inputs embedded on the host; against torch autograd over the float64 oracle at the project's bars for
that kernel (tests/test_gpu_grad.py: BAR_P, BAR_Z = 4 x the measurements of profiles/r03_grad_errors.json -- the
arithmetic is that kernel's on a zero-padded problem); launch counters, reproducibility, overflow recovery, graph capture
and the route through ConditionalDensityEstimator."""
import contextlib
import math

import numpy as np
import pytest
import torch

from conftest import grad_err
import test_padded_train_host as HT

from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
BAR_P, BAR_Z = 5e-5, 5e-6  # tests/test_gpu_grad.py

# (D, S, L, U, M_z, M_p, N): odd and even widths in both layouts, one row and several, N of one sample, a partial tile
# and several workgroups, the largest S at D = 5 (L = 2 and L = 1) and D = 47
SHAPES = [(2, 1, 1, 15, 1, 1, 1), (3, 2, 2, 16, 3, 1, 17), (5, 8, 2, 15, 3, 3, 33), (31, 1, 3, 15, 1, 1, 1000),
          (33, 2, 1, 16, 2, 2, 40), (63, 4, 2, 15, 1, 1, 4097), (5, 14, 1, 16, 2, 1, 50), (47, 4, 2, 15, 1, 1, 100),
          (47, 6, 1, 15, 2, 2, 33)]
COUNTERS = range(5)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@contextlib.contextmanager
def float64():
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


@contextlib.contextmanager
def recovery(tnf, mode):
    fn = tnf.padtrain_ops._FlowPaddedLogProbFn
    before = fn.overflow_recovery
    fn.overflow_recovery = mode
    try:
        yield fn
    finally:
        fn.overflow_recovery = before


def counts():
    torch.cuda.synchronize()
    return ([lib.tnf_diag_launch_count(f) for f in range(L_.DIAG_FAMILIES)],
            [lib.tnf_padtrain_launch_count(w) for w in COUNTERS])


def launched(before):
    diag, pad = counts()
    return ({f: a - b for f, (a, b) in enumerate(zip(diag, before[0])) if a != b},
            [a - b for a, b in zip(pad, before[1])])


def feature_slots(D):
    """embedded feature index of every real feature, from the restated layout"""
    emb = HT.embed_features(np.arange(D), D, fill=-1)
    slots = np.empty(D, dtype=np.int64)
    slots[emb[emb >= 0]] = np.nonzero(emb >= 0)[0]
    return torch.from_numpy(slots).cuda()


def flow_inputs(D, S, L, U, Mz, Mp, N, seed):
    """tests/test_gpu_domain.py's pattern: parameter rows, frozen statistics, samples (float32) and loss weights."""
    rng = np.random.RandomState(seed)
    k = min(1.0, math.sqrt(4.0 / S))
    P = lib.tnf_flow_num_params(D, S, L, U)
    params = torch.from_numpy(rng.normal(0.0, 0.1 * k, (Mp, P)).astype(np.float32))
    mean = torch.from_numpy(rng.normal(0.0, 0.3 * k, (2 * S, D)).astype(np.float32))
    alpha = torch.from_numpy(np.exp(rng.normal(0.0, 0.2 * k, (2 * S, D))).astype(np.float32))
    z = torch.from_numpy(rng.normal(0.0, 1.0, (Mz, N, D)).astype(np.float32))
    w = torch.from_numpy(rng.normal(0.0, 1.0, (Mz, N)).astype(np.float32))
    return params, mean, alpha, z, w


def make_flow(tnf, D, S, L, U, mean, alpha, switch=True):
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    for b, m, a in zip(nf._bn_layers(), mean, alpha):
        b.set_last_stats(m.cuda(), a.cuda())
    nf.padded_training = switch
    return nf


# ---- the four kernels alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 17, 4097])
@pytest.mark.parametrize("D", [2, 3, 5, 31, 33, 63])
def test_row_kernels_are_torch_indexing(tnf, D, R):
    """embed_rows / gather_rows, the real side at a pointer 4 bytes off a 16-byte boundary: bit-equal to indexing with
    the feature map; embed writes its own zeros (the output starts as NaN) and nothing beyond the rows."""
    W, slots = 2 * HT.half(D), feature_slots(D)
    g = torch.Generator(device="cuda").manual_seed(D * 7919 + R)
    base = torch.randn(R * D + 1, device="cuda", generator=g)
    rows = base[1:].view(R, D)
    assert rows.data_ptr() % 16 == 4
    out = torch.full((R * W + 64,), float("nan"), device="cuda")
    L_.check(lib.tnf_flow_padded_embed_rows_f32(rows.data_ptr(), out.data_ptr(), R, D, L_.stream_ptr()))
    want = torch.zeros(R, W, device="cuda")
    want[:, slots] = rows
    assert torch.equal(out[:R * W].view(R, W), want)
    assert bool(torch.isnan(out[R * W:]).all())
    assert torch.equal(tnf.padtrain_ops.embed_rows_raw(rows.contiguous(), D), want)
    # gather: the padding is not read back (it holds other numbers here), the real side again 4 bytes off
    emb = torch.randn(R, W, device="cuda", generator=g)
    back = torch.full((R * D + 65,), 7.0, device="cuda")
    L_.check(lib.tnf_flow_padded_gather_rows_f32(emb.data_ptr(), back.data_ptr() + 4, R, D, L_.stream_ptr()))
    assert torch.equal(back[1:R * D + 1].view(R, D), emb[:, slots])
    assert float(back[0]) == 7.0 and bool((back[R * D + 1:] == 7.0).all())
    assert torch.equal(tnf.padtrain_ops.gather_rows_raw(emb, D), emb[:, slots])


@pytest.mark.parametrize("Mp", [1, 3])
@pytest.mark.parametrize("D,S,L,U", [(2, 2, 2, 15), (3, 1, 3, 16), (5, 8, 2, 15), (31, 2, 1, 15), (33, 2, 2, 16),
                                     (63, 4, 2, 15)])
def test_param_kernels_are_torch_indexing(tnf, oracle, D, S, L, U, Mp):
    """embed_params / gather_params with rows longer than the flow's and pointers 4 bytes off a 16-byte boundary:
    bit-equal to indexing with the restated map; padding is 0 (parameters), 0 / 1 (mean / alpha); gather reads only the
    real slots and leaves the tail of each output row alone."""
    W, slots = 2 * HT.half(D), feature_slots(D)
    e = torch.from_numpy(HT.index_map(D, S, L, U, oracle)).cuda()
    P, Pe = e.numel(), lib.tnf_flow_num_params(W, S, L, U)
    stride = P + 3
    g = torch.Generator(device="cuda").manual_seed(D * 31 + Mp)
    base = torch.randn(Mp * stride + 1, device="cuda", generator=g)
    params = base[1:].view(Mp, stride)
    sbase = torch.randn(2, 2 * S * D + 1, device="cuda", generator=g)
    mean, alpha = sbase[0, 1:].view(2 * S, D), sbase[1, 1:].view(2 * S, D)
    outs = [torch.full((n + 64,), float("nan"), device="cuda") for n in (Mp * Pe, 2 * S * W, 2 * S * W)]
    assert params.data_ptr() % 16 == 4 and mean.data_ptr() % 16 == 4
    L_.check(lib.tnf_flow_padded_embed_params_f32(params.data_ptr(), mean.data_ptr(), alpha.data_ptr(), outs[0].data_ptr(),
                                                  outs[1].data_ptr(), outs[2].data_ptr(), Mp, D, S, L, U, stride,
                                                  L_.stream_ptr()))
    want_p = torch.zeros(Mp, Pe, device="cuda")
    want_p[:, e] = params[:, :P]
    want_m, want_a = torch.zeros(2 * S, W, device="cuda"), torch.ones(2 * S, W, device="cuda")
    want_m[:, slots], want_a[:, slots] = mean, alpha
    for out, want in zip(outs, (want_p, want_m, want_a)):
        assert torch.equal(out[:want.numel()].view(want.shape), want)
        assert bool(torch.isnan(out[want.numel():]).all())
    grads = torch.randn(Mp, Pe, device="cuda", generator=g)  # the padded slots hold numbers too
    back = torch.full((Mp * stride + 65,), 7.0, device="cuda")
    L_.check(lib.tnf_flow_padded_gather_params_f32(grads.data_ptr(), back.data_ptr() + 4, Mp, D, S, L, U, stride,
                                                   L_.stream_ptr()))
    got = back[1:Mp * stride + 1].view(Mp, stride)
    assert torch.equal(got[:, :P], grads[:, e])
    assert bool((got[:, P:] == 7.0).all()) and float(back[0]) == 7.0 and bool((back[Mp * stride + 1:] == 7.0).all())


# ---- the route, each shape computed once ---------------------------------------------------------------------------------
_RESULTS = {}


def results(tnf, oracle, shape):
    """One training step per shape through (a) the route, (b) the existing reversible pair at width 2H on inputs embedded
    on the host, (c) torch autograd over the float64 oracle; computed once and shared by the tests below."""
    if shape in _RESULTS:
        return _RESULTS[shape]
    D, S, L, U, Mz, Mp, N = shape
    W = 2 * HT.half(D)
    params, mean, alpha, z0, w = flow_inputs(D, S, L, U, Mz, Mp, N, seed=sum(shape))
    out = {}
    # (a)
    nf = make_flow(tnf, D, S, L, U, mean, alpha)
    p, z = params.cuda().requires_grad_(), z0.cuda().requires_grad_()
    assert tnf.padtrain_ops.flow_padded_train_supported(Mz, Mp, N, D, S, L, U) and nf._train_path(z, p) == "padded"
    before = counts()
    lp = nf.log_prob(z, p)
    loss = (lp * w.cuda()).sum() / N
    loss.backward()
    out["launched"] = launched(before)
    out["route"] = (lp.detach(), loss.detach(), p.grad, z.grad)
    with torch.no_grad():
        out["lp_nograd"] = nf.log_prob(z0.cuda(), params.cuda())
    # (b): embedded on the host with the restated layout
    pe = torch.from_numpy(np.stack([HT.embed_row(r, D, S, L, U, oracle) for r in params.numpy()])).cuda().requires_grad_()
    ze = torch.from_numpy(HT.embed_features(z0.numpy(), D)).cuda().requires_grad_()
    mean_e = torch.from_numpy(HT.embed_features(mean.numpy(), D, 0.0)).cuda()
    alpha_e = torch.from_numpy(HT.embed_features(alpha.numpy(), D, 1.0)).cuda()
    assert tnf.ops.flow_train_rev_supported(Mz, Mp, N, W, S, L, U)
    lpe = tnf.ops.flow_log_prob_train(ze, pe, mean_e, alpha_e, W, S, L, U, reversible=True)
    ((lpe * w.cuda()).sum() / N).backward()
    out["pair"] = (pe.grad, ze.grad)
    # (c)
    with float64():
        p_ref, z_ref = params.double().requires_grad_(), z0.double().requires_grad_()
        stats = [(m.double(), a.double()) for m, a in zip(mean, alpha)]
        loss_ref = (oracle.flow_log_prob(z_ref, p_ref, D, S, L, U, stats) * w.double()).sum() / N
        loss_ref.backward()
    out["oracle"] = (loss_ref.detach(), p_ref.grad, z_ref.grad)
    _RESULTS[shape] = out
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_route_is_the_existing_pair_at_the_embedded_width_bit_for_bit(tnf, oracle, shape):
    D, S, L, U = shape[:4]
    r = results(tnf, oracle, shape)
    lp, _, gp, gz = r["route"]
    assert torch.equal(lp, r["lp_nograd"])  # the forward value is the no-grad route's
    e = torch.from_numpy(HT.index_map(D, S, L, U, oracle)).cuda()
    gpe, gze = r["pair"]
    assert torch.equal(gp, gpe[:, e])
    assert torch.equal(gz, gze[..., feature_slots(D)])
    assert bool(torch.isfinite(gp).all()) and float(gp.abs().max()) > 0 and float(gz.abs().max()) > 0


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_route_against_the_float64_oracle(tnf, oracle, shape):
    r = results(tnf, oracle, shape)
    _, loss, gp, gz = r["route"]
    loss_ref, gp_ref, gz_ref = r["oracle"]
    err = [float((g.cpu().double() - ref).abs().max() / ref.abs().max()) for g, ref in ((gp, gp_ref), (gz, gz_ref))]
    print("shape %s: loss %.9g vs %.9g, d params %.3e, d z %.3e of the largest entry" % (
        shape, float(loss), float(loss_ref), err[0], err[1]))  # each figure, before anything is asserted
    torch.testing.assert_close(loss.cpu().double(), loss_ref, rtol=1e-5, atol=0.0)
    grad_err("log_prob training, padded pair: d params", gp, gp_ref, BAR_P)
    grad_err("log_prob training, padded pair: d z", gz, gz_ref, BAR_Z)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_launches_of_a_step(tnf, oracle, shape):
    """"device" recovery (the default): one padded forward, one reversible backward, no generic backward kernel; the
    composite once, its embed / gather kernels once for the step and once more for the gated recomputation -- which
    exists only where the per-layer pair does (32 samples per row)."""
    D, S, L, U, Mz, Mp, N = shape
    diag, pad = results(tnf, oracle, shape)["launched"]
    assert diag.get(L_.DIAG_FLOW_PADDED) == 1 and diag.get(L_.DIAG_BWD_FLOW_REV) == 1
    assert L_.DIAG_BWD_GENERIC not in diag and L_.DIAG_BWD_LAYER_F16 not in diag
    assert not set(diag) & {L_.DIAG_FLOW_FUSED2, L_.DIAG_FLOW_FUSED3, L_.DIAG_FLOW_F16, L_.DIAG_FLOW_FP32,
                            L_.DIAG_FLOW_PADDED_FWD}
    twice = 2 if tnf.ops.flow_train_supported(Mz, Mp, N, 2 * HT.half(D), S, L, U) else 1
    assert pad == [twice, twice, twice, twice, 1], pad


def test_launches_without_recovery_and_with_a_constant_z(tnf):
    """"off": the step is the padded forward and the composite's five launches plus the backward's own; a constant z
    skips g_z (no gather_rows) and leaves the parameter gradient bit for bit what it is with it."""
    D, S, L, U, N = 5, 4, 2, 15, 300
    params, mean, alpha, z0, w = flow_inputs(D, S, L, U, 1, 1, N, seed=5)
    nf = make_flow(tnf, D, S, L, U, mean, alpha)
    grads = []
    with recovery(tnf, "off"):
        for z_grad in (True, False):
            p, z = params.cuda().requires_grad_(), z0.cuda().requires_grad_(z_grad)
            before = counts()
            ((nf.log_prob(z, p) * w.cuda()).sum() / N).backward()
            diag, pad = launched(before)
            assert diag == {L_.DIAG_FLOW_PADDED: 1, L_.DIAG_BWD_FLOW_REV: 1}, diag
            assert pad == [1, int(z_grad), 1, 1, 1], pad
            assert z.grad is not None if z_grad else z.grad is None
            grads.append(p.grad.clone())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("shape", [(5, 8, 2, 15, 3, 3, 33), (47, 4, 2, 15, 2, 1, 777)], ids=str)
def test_backward_is_reproducible_bit_for_bit(tnf, shape):
    D, S, L, U, Mz, Mp, N = shape
    params, mean, alpha, z0, w = flow_inputs(D, S, L, U, Mz, Mp, N, seed=11)
    nf = make_flow(tnf, D, S, L, U, mean, alpha)
    runs = []
    for _ in range(3):
        p, z = params.cuda().requires_grad_(), z0.cuda().requires_grad_()
        ((nf.log_prob(z, p) * w.cuda()).sum() / N).backward()
        runs.append((p.grad.clone(), z.grad.clone()))
    for gp, gz in runs[1:]:
        assert torch.equal(gp, runs[0][0]) and torch.equal(gz, runs[0][1])
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].abs().max()) > 0


def test_zero_upstream_gives_exactly_zero(tnf):
    D, S, L, U, N = 7, 2, 2, 15, 100
    params, mean, alpha, z0, _ = flow_inputs(D, S, L, U, 1, 1, N, seed=3)
    nf = make_flow(tnf, D, S, L, U, mean, alpha)
    p, z = params.cuda().requires_grad_(), z0.cuda().requires_grad_()
    (nf.log_prob(z, p) * 0.0).sum().backward()
    assert bool((p.grad == 0).all()) and bool((z.grad == 0).all())


def test_overflow_recovery(tnf, oracle):
    """The input pattern of tests/test_gpu_grad.py::test_flow_reversible_backward_overflow_falls_back (a few rows 3000
    sigma out) at D = 5, N = 4096, at that test's tolerances: "host" and "device" set the flag and match torch autograd
    over the oracle, "off" yields NaN; a well-behaved batch leaves the flag clear and the one-kernel result in place."""
    D, S, L, U, N = 5, 4, 2, 15, 4096
    rng = np.random.RandomState(1)
    P = lib.tnf_flow_num_params(D, S, L, U)
    p0 = torch.tensor(rng.normal(0, 0.05, (1, P))).float()
    mean, alpha = torch.zeros(2 * S, D), torch.ones(2 * S, D)
    nf = make_flow(tnf, D, S, L, U, mean, alpha)
    z0 = torch.tensor(rng.normal(0, 1, (1, N, D))).float()
    z0[0, ::512] *= 3000.0
    with float64():
        p_ref = p0.double().requires_grad_()
        stats = [(m.double(), a.double()) for m, a in zip(mean, alpha)]
        (-oracle.flow_log_prob(z0.double(), p_ref, D, S, L, U, stats).sum()).backward()
    scale = float(p_ref.grad.abs().max())
    want = (p_ref.grad / scale).float()
    z = z0.cuda()
    with recovery(tnf, "host") as fn:
        before = fn.overflow_fallbacks
        p = p0.cuda().requires_grad_()
        assert nf._train_path(z, p) == "padded"
        (-nf.log_prob(z, p).sum()).backward()
        assert fn.overflow_fallbacks == before + 1 and int(fn.last_overflow_flag.item()) == 1
        assert bool(torch.isfinite(p.grad).all())
        torch.testing.assert_close(p.grad.cpu() / scale, want, rtol=2e-3, atol=2e-5)
        g_host = p.grad.clone()
    with recovery(tnf, "device") as fn:
        p, zg = p0.cuda().requires_grad_(), z.clone().requires_grad_()
        (-nf.log_prob(zg, p).sum()).backward()
        assert int(fn.last_overflow_flag.item()) == 1
        torch.testing.assert_close(p.grad / scale, g_host / scale, rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(p.grad.cpu() / scale, want, rtol=2e-3, atol=2e-5)
        assert bool(torch.isfinite(zg.grad).all())
    z_ok = torch.tensor(rng.normal(0, 1, (1, N, D))).float().cuda()
    grads = []
    for mode in ("device", "off"):
        with recovery(tnf, mode) as fn:
            p, zg = p0.cuda().requires_grad_(), z_ok.clone().requires_grad_()
            (-nf.log_prob(zg, p).sum()).backward()
            grads.append((p.grad.clone(), zg.grad.clone()))
            if mode == "device":
                assert int(fn.last_overflow_flag.item()) == 0
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    with recovery(tnf, "off"):
        p = p0.cuda().requires_grad_()
        (-nf.log_prob(z, p).sum()).backward()
        assert bool(torch.isnan(p.grad).any())


def test_graph_captured_step_equals_the_eager_step(tnf):
    """A D = 4 training step (loss, backward, Adam with capturable=True) captured on a side stream and replayed moves the
    parameters as the eager steps do: every kernel of the route is capturable, and its gradient is reproducible."""
    from torch_nf_amd.graphs import GraphedStep

    D, S, L, U, N = 4, 4, 2, 15, 2048
    params, mean, alpha, z0, _ = flow_inputs(D, S, L, U, 1, 1, N, seed=4)
    z = z0.cuda()
    res = {}
    for mode in ("eager", "graph"):
        nf = tnf.NormFlow(D, False, "coupling", S, L, U)
        nf.padded_training = True
        for b, m, a in zip(nf._bn_layers(), mean, alpha):
            b.set_last_stats(m.cuda(), a.cuda())
        nf.params = params.clone().cuda().requires_grad_()
        opt = torch.optim.Adam([nf.params], lr=1e-3, capturable=True)
        assert nf._train_path(z, nf.params) == "padded"

        def step():
            opt.zero_grad(set_to_none=True)
            loss = -nf.log_prob(z).mean()
            loss.backward()
            opt.step()
            return loss.detach()

        before = counts()
        if mode == "eager":
            ls = [step().item() for _ in range(8)]
        else:
            gs = GraphedStep(step, warmup=3)
            ls = [w.item() for w in gs.warmup_outputs] + [gs().item() for _ in range(5)]
        diag, pad = launched(before)
        assert diag.get(L_.DIAG_BWD_FLOW_REV) == (8 if mode == "eager" else 4) and L_.DIAG_BWD_GENERIC not in diag
        res[mode] = (np.array(ls), nf.params.detach().cpu())
    assert ls[-1] < ls[0]
    np.testing.assert_array_equal(res["graph"][0], res["eager"][0])
    assert torch.equal(res["graph"][1], res["eager"][1])


def test_through_the_conditional_density_estimator(tnf):
    """ConditionalDensityEstimator.log_prob with 32 atoms per context at D = 4 (per-context parameter rows): the
    gradients of param_net with the switch on match the switch-off route (one kernel per bijector) to the bars."""
    torch.manual_seed(3)
    D, S, L, U, M, N, Dx = 4, 2, 2, 15, 8, 32, 3
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    cde = tnf.ConditionalDensityEstimator(nf, Dx, [32, 32])
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(M, Dx, device="cuda", generator=g)
    z = torch.randn(M, N, D, device="cuda", generator=g)
    w = torch.randn(M, N, device="cuda", generator=g)
    got = {}
    for switch in (False, True):
        nf.padded_training = switch
        cde.param_net.zero_grad(set_to_none=True)
        before = counts()
        lp = cde.log_prob(z, x)
        ((lp * w).sum() / N).backward()
        diag, pad = launched(before)
        assert (diag.get(L_.DIAG_BWD_FLOW_REV, 0), pad[4]) == ((1, 1) if switch else (0, 0)), (switch, diag, pad)
        got[switch] = (lp.detach(), torch.cat([q.grad.reshape(-1) for q in cde.param_net.parameters()]))
    torch.testing.assert_close(got[True][0], got[False][0], rtol=1e-5, atol=1e-5)
    grad_err("padded training through the CDE: d param_net", got[True][1], got[False][1], BAR_P)
