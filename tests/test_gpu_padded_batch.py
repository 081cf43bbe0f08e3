"""Sampling coupling flows of width 2 <= D <= 63 with fresh batch statistics through the chains at the embedded width
(include/tnf_padbatch.h, NormFlow.padded_batch_forward) on the GPU: the pad-aware fold kernel alone against the existing
fold on the same columns; the no-autograd chain against the per-bijector composition; the one-node autograd pair against
the per-bijector autograd route, torch autograd over the float64-capable oracle and finite differences; the padded gradient
columns; and train_efn at the width the reference trains, eager and as one captured graph.

The bars are the project's own for the same arithmetic at D = 32 / 64: those of
test_gpu_parity.test_batch_stats_forward_one_call_vs_per_bijector and of test_gpu_grad._one_node_body with BAR_FWD."""
import numpy as np
import pytest
import torch

from conftest import grad_err
from test_gpu_grad import BAR_FWD

pytestmark = pytest.mark.gpu

PB_FOLD, PB_STATS, PB_FORWARD, PB_TRAIN_FWD, PB_TRAIN_BWD = range(5)  # include/tnf_padbatch.h


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available()
    return torch_nf_amd


def counts(tnf):
    return [tnf._lib.lib.tnf_padbatch_launch_count(w) for w in range(5)]


def real_slots(D):
    """Embedded feature of every real feature: f -> f for f < h, else H + (f - h)."""
    H, h = (16 if D <= 31 else 32), D // 2
    return torch.tensor([f if f < h else H + f - h for f in range(D)])


# ---- 1. the fold kernel alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("D,Mp,layer", [(2, 1, 0), (5, 3, 1), (16, 1, 1), (31, 2, 2), (33, 3, 3), (63, 1, 1)])
def test_fold_kernel_against_the_existing_fold(tnf, D, Mp, layer, eps):
    """Real slots: bit-equal to flow_batch_finalize_fold_kernel (through tnf_flow_forward_batch_fold_f32 at width 2H) fed
    the same columns.  Padded slots: exactly (mean, alpha, A, B) = (0, 1, 1, 0), whatever the moments there say."""
    from torch_nf_amd import padbatch_ops, padtrain_ops

    lib, check = tnf._lib.lib, tnf._lib.check
    S, L, U, R = 2, 2, 15, 37
    W = padtrain_ops.padded_width(D)
    slots = real_slots(D).cuda()
    pad = torch.ones(W, dtype=torch.bool, device="cuda")
    pad[slots] = False
    gen = torch.Generator(device="cuda").manual_seed(7 * D + layer)
    rows = torch.randn(R, D, device="cuda", generator=gen) * 1.7 + 0.4
    xe = padtrain_ops.embed_rows_raw(rows, D)
    moments = torch.empty(2 * W + 1, dtype=torch.float64, device="cuda")
    check(lib.tnf_bn_batch_moments_f32(xe.data_ptr(), moments.data_ptr(), R, W, tnf._lib.stream_ptr()))
    assert float(moments[2 * W]) == R and bool((moments[:2 * W][torch.cat((pad, pad))] == 0).all())
    P = lib.tnf_flow_num_params(D, S, L, U)
    params = torch.randn(Mp, P, device="cuda", generator=gen) * 0.3
    stats = torch.zeros(2 * S, D, device="cuda")
    pe, _, _ = padtrain_ops.embed_params_raw(params, P, stats, stats + 1, D, S, L, U)
    stage = lib.tnf_flow_num_params(W, 1, L, U)
    affine_off = (layer >> 1) * stage + lib.tnf_coupling_num_params(W, L, U, 1) + lib.tnf_coupling_num_params(W, L, U, 0)
    before = counts(tnf)
    mean, alpha, fold, ldc = padbatch_ops.padded_batch_fold_raw(pe, moments, D, affine_off, layer & 1, True, eps)
    assert counts(tnf)[PB_FOLD] == before[PB_FOLD] + 1
    # the existing kernel on the same real columns; its padded columns get unit-variance moments so that it stays finite
    m_old = moments.clone()
    m_old[W:2 * W][pad] = float(R)
    nbytes = check(lib.tnf_flow_forward_batch_workspace_bytes(Mp, W, S, L))
    ws = torch.zeros(nbytes // 4 + 1, dtype=torch.float32, device="cuda")
    mean_o = torch.empty(2 * S, W, device="cuda")
    alpha_o = torch.empty(2 * S, W, device="cuda")
    check(lib.tnf_flow_forward_batch_fold_f32(layer, pe.data_ptr(), m_old.data_ptr(), mean_o.data_ptr(), alpha_o.data_ptr(),
                                              Mp, W, S, L, U, pe.shape[1], eps, ws.data_ptr(), nbytes, tnf._lib.stream_ptr()))
    fold_o = ws[:Mp * 2 * W].view(Mp, 2, W)  # the workspace opens with fold (Mp, 2, W) | ldc (Mp)
    assert torch.equal(mean[slots], mean_o[layer][slots]) and torch.equal(alpha[slots], alpha_o[layer][slots])
    assert torch.equal(fold[:, :, slots], fold_o[:, :, slots])
    assert bool((mean[pad] == 0).all()) and bool((alpha[pad] == 1).all())
    assert bool((fold[:, 0, pad] == 1).all()) and bool((fold[:, 1, pad] == 0).all())
    assert bool(torch.isfinite(fold).all()) and bool(torch.isfinite(ldc).all())
    # the constant log-det: the real columns' terms only, a float32 sum of at most 2 * 63 of them
    terms = -torch.log(alpha[slots].double())[None, :].expand(Mp, D)
    if layer & 1:
        terms = torch.cat((terms, pe[:, affine_off:affine_off + W][:, slots].double()), 1)
    want = terms.sum(1)
    assert float((ldc.double() - want).abs().max()) <= 2.0 ** -24 * 128 * float(terms.abs().sum(1).max() + 1.0)
    # first = 0 adds to what is there
    _, _, _, ldc2 = padbatch_ops.padded_batch_fold_raw(pe, moments, D, affine_off, layer & 1, False, eps, ldc=ldc.clone())
    torch.testing.assert_close(ldc2, 2 * ldc, rtol=1e-6, atol=1e-6)


# ---- 2. the no-autograd chain -------------------------------------------------------------------------------------------------
CHAIN_CASES = [(2, 1, 1, 15, 1, 2), (2, 2, 3, 16, 3, 32), (5, 2, 2, 15, 1, 33), (5, 1, 1, 16, 2, 40), (16, 1, 2, 16, 1, 2),
               (16, 2, 1, 15, 3, 32), (31, 2, 3, 15, 1, 33), (31, 1, 2, 16, 2, 40), (33, 1, 3, 16, 1, 2),
               (33, 2, 2, 15, 1, 33), (63, 2, 1, 16, 3, 32), (63, 1, 2, 15, 2, 40)]


def _chain_pair(tnf, nf, omega, params):
    out = {}
    for on in (True, False):
        nf.padded_batch_forward = on
        before = counts(tnf)
        with torch.no_grad():
            z, lq = nf._forward_from(omega, params, freeze_bn=False)
        ran = [a - b for a, b in zip(counts(tnf), before)]
        S2 = 2 * nf.num_stages
        assert ran == ([S2, 1, 1, 0, 0] if on else [0] * 5), (on, ran)  # the new entry ran, and only with the switch
        out[on] = (z, lq, [b.get_last_mean().clone() for b in nf._bn_layers()],
                   [b.get_last_alpha().clone() for b in nf._bn_layers()])
    return out


@pytest.mark.parametrize("D,S,L,U,M,N", CHAIN_CASES)
def test_chain_vs_per_bijector(tnf, D, S, L, U, M, N):
    """NormFlow.forward(freeze_bn=False) without autograd: tnf_flow_padded_forward_batch_f32 against the per-bijector
    composition (switch off) -- samples, log-densities and the (D,) statistics every BatchNorm layer caches -- and the
    density log_prob assigns to the samples afterwards."""
    rng = np.random.RandomState(D + N)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    params = torch.tensor(rng.normal(0, 0.1, (M, nf.D_params))).float().cuda()
    omega = rng.normal(0, 1, (M, N, D))
    out = _chain_pair(tnf, nf, omega, params)
    assert out[True][0].shape == (M, N, D) and out[True][1].dtype == torch.float64
    torch.testing.assert_close(out[True][0], out[False][0], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(out[True][1], out[False][1], rtol=1e-6, atol=2e-4)
    for a, b in zip(out[True][2] + out[True][3], out[False][2] + out[False][3]):
        assert a.shape == (D,)
        torch.testing.assert_close(a.cpu(), b.cpu(), rtol=2e-5, atol=2e-5)
    # the cached statistics serve the frozen paths afterwards
    with torch.no_grad():
        lp = nf.log_prob(out[True][0], params)
    torch.testing.assert_close(lp.double(), out[True][1], rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("D,M,N", [(2, 1, 33), (5, 3, 32), (33, 2, 40), (63, 1, 33)])
def test_chain_with_eps_zero_stays_finite(tnf, D, M, N):
    """BatchNorm(eps=0): the existing fold on a padded column would form 0 * inf.  Everything stays finite and equals
    the per-bijector composition."""
    S, L, U = 2, 2, 15
    rng = np.random.RandomState(D)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    for b in nf._bn_layers():
        b.eps = 0.0
    params = torch.tensor(rng.normal(0, 0.1, (M, nf.D_params))).float().cuda()
    out = _chain_pair(tnf, nf, rng.normal(0, 1, (M, N, D)), params)
    for t in (out[True][0], out[True][1]) + tuple(out[True][2]) + tuple(out[True][3]):
        assert bool(torch.isfinite(t).all())
    torch.testing.assert_close(out[True][0], out[False][0], rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(out[True][1], out[False][1], rtol=1e-6, atol=2e-4)
    for a, b in zip(out[True][2] + out[True][3], out[False][2] + out[False][3]):
        torch.testing.assert_close(a.cpu(), b.cpu(), rtol=2e-5, atol=2e-5)


# ---- 3. the one-node pair -----------------------------------------------------------------------------------------------------
def _one_node_body(tnf, oracle, nf, p0, om0, w, D, S, L, U):
    """test_gpu_grad._one_node_body with the switch `padded_batch_forward` in the place of `fused_batch_forward` and the
    node of padbatch_ops in the place of ops.flow_forward_train; its bars."""
    from torch_nf_amd import padbatch_ops

    res = {}
    for fused in (True, False):
        nf.padded_batch_forward = fused
        before = counts(tnf)
        p = p0.clone().cuda().requires_grad_()
        z, lq = nf._forward_from(om0.cuda(), p, freeze_bn=False)  # the base draw is a constant of this call
        loss = (lq * w.cuda()).mean() + (z ** 2).mean()
        loss.backward()
        ran = [a - b for a, b in zip(counts(tnf), before)]
        assert ran == ([2 * S, 1, 0, 1, 1] if fused else [0] * 5), (fused, ran)  # the launch counters: the new pair ran
        res[fused] = (loss.detach().cpu(), p.grad.cpu(), [b.get_last_alpha().cpu().clone() for b in nf._bn_layers()])
    # the node itself also differentiates w.r.t. the base draw
    p = p0.clone().cuda().requires_grad_()
    om = om0.clone().cuda().requires_grad_()
    z, sld, _, _ = padbatch_ops.flow_padded_forward_train(om, p, D, S, L, U, 1e-5)
    lq = tnf.ops.base_log_density_f64(om.detach()) - sld
    ((lq * w.cuda()).mean() + (z ** 2).mean()).backward()
    p_ref = p0.clone().requires_grad_()
    z_r, lq_r, _ = oracle.flow_forward(om0.double().numpy(), p_ref, D, S, L, U, None)
    loss_r = (lq_r * w).mean() + (z_r ** 2).mean()
    loss_r.backward()
    sp = float(p_ref.grad.abs().max())
    torch.testing.assert_close(res[True][0], res[False][0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(res[True][0].double(), loss_r.detach().double(), rtol=1e-5, atol=1e-5)
    for a, b in zip(res[True][2], res[False][2]):
        torch.testing.assert_close(a, b, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(res[True][1], res[False][1], rtol=1e-3, atol=1e-4 * sp)
    torch.testing.assert_close(res[True][1], p_ref.grad, rtol=5e-3, atol=2e-4 * sp)
    torch.testing.assert_close(p.grad.cpu(), p_ref.grad, rtol=5e-3, atol=2e-4 * sp)
    name = "sampling with fresh statistics at D=%d S=%d L=%d U=%d, " % (D, S, L, U)
    print(name + "one-node padded chain %.3e, per-bijector %.3e of the largest entry" % (
        grad_err(name + "one-node padded chain: d params", res[True][1], p_ref.grad),
        grad_err(name + "per-bijector: d params", res[False][1], p_ref.grad)))
    grad_err("sampling with fresh statistics, one-node padded chain: d params", res[True][1], p_ref.grad, BAR_FWD)
    grad_err("sampling with fresh statistics, per-bijector (padded widths): d params", res[False][1], p_ref.grad, BAR_FWD)
    # d loss / d omega: finite differences of the oracle along one random direction (the oracle takes omega as numpy)
    dirn = torch.tensor(np.random.RandomState(1).normal(0, 1, om0.shape)).float()
    h = 1e-3

    def oracle_loss(o):
        zz, ll, _ = oracle.flow_forward(o.double().numpy(), p0, D, S, L, U, None)
        # the base density is a function of omega too; the node returns only z and sum_log_det, so compare that part
        base = torch.tensor(oracle.base_log_density_f64(o.double().numpy()))
        return float((((ll - base) * w).mean() + (zz ** 2).mean()).double())

    fd = (oracle_loss(om0 + h * dirn) - oracle_loss(om0 - h * dirn)) / (2 * h)
    got = float((om.grad.cpu() * dirn).sum())
    assert abs(got - fd) <= 2e-2 * max(1.0, abs(fd)), (got, fd)


NODE_CASES = [(2, 1, 1, 15, 1, 33), (2, 2, 2, 16, 2, 40), (5, 2, 3, 15, 3, 32), (5, 1, 2, 16, 1, 33), (16, 2, 1, 16, 2, 40),
              (16, 1, 3, 16, 1, 33), (31, 1, 2, 15, 3, 32), (31, 2, 1, 16, 1, 33), (33, 2, 2, 15, 2, 40),
              (33, 1, 3, 16, 3, 32), (63, 1, 1, 15, 1, 33), (63, 2, 2, 16, 2, 40)]


@pytest.mark.parametrize("D,S,L,U,M,N", NODE_CASES)
def test_one_node_pair(tnf, oracle, D, S, L, U, M, N):
    """Sampling with fresh batch statistics under autograd as ONE node at the embedded width
    (tnf_flow_padded_forward_train_fwd_f32 / _bwd_f32): loss and gradients w.r.t. the parameter rows and the base draw
    against (a) the per-bijector autograd route and (b) torch autograd over the oracle."""
    rng = np.random.RandomState(D + N)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    p0 = torch.tensor(rng.normal(0, 0.1, (M, nf.D_params))).float()
    om0 = torch.tensor(rng.normal(0, 1, (M, N, D))).float()
    w = torch.tensor(rng.uniform(0.5, 1.5, (M, N))).float()
    _one_node_body(tnf, oracle, nf, p0, om0, w, D, S, L, U)


@pytest.mark.parametrize("fp32_bwd", [0, 1])
@pytest.mark.parametrize("D,S,L,U,M,N", [(5, 2, 2, 15, 2, 40), (33, 1, 2, 16, 1, 33)])
def test_padded_gradient_columns_stay_zero(tnf, D, S, L, U, M, N, fp32_bwd):
    """The backward needs no arithmetic of its own: the existing tnf_flow_forward_train_bwd_f32 at width 2H, on the states
    and folds the padded forward kept and on host-embedded inputs, leaves the padded columns of g_omega at exactly 0 -- with
    (0, 1) at padding P = Q = 0 and v = 0 there -- and its real columns and parameter gradients are the composite's."""
    from torch_nf_amd import padbatch_ops, padtrain_ops

    lib, check = tnf._lib.lib, tnf._lib.check
    W = padtrain_ops.padded_width(D)
    slots = real_slots(D).cuda()
    pad = torch.ones(W, dtype=torch.bool, device="cuda")
    pad[slots] = False
    gen = torch.Generator(device="cuda").manual_seed(D)
    P = lib.tnf_flow_num_params(D, S, L, U)
    p = (torch.randn(M, P, device="cuda", generator=gen) * 0.1).requires_grad_()
    om = torch.randn(M, N, D, device="cuda", generator=gen).requires_grad_()
    gz = torch.randn(M, N, D, device="cuda", generator=gen)
    gs = torch.randn(M, N, device="cuda", generator=gen)
    check(lib.tnf_set_option(tnf._lib.OPT_TRAIN_BWD_FP32, fp32_bwd))
    try:
        z, sld, mean, alpha = padbatch_ops.flow_padded_forward_train(om, p, D, S, L, U, 1e-5)
        states, folds = z.grad_fn.saved_tensors[2:4]
        assert states.shape == (2 * S, M, N, W) and folds.shape == (2 * S, M, 2, W)
        assert bool((states[..., pad] == 0).all())  # the padding stays exactly 0 through every layer
        assert bool((folds[:, :, 0, pad] == 1).all()) and bool((folds[:, :, 1, pad] == 0).all())
        torch.autograd.backward((z, sld), (gz, gs))
        # the existing backward on the embedded problem
        pe, mean_e, alpha_e = padtrain_ops.embed_params_raw(p.detach(), P, mean, alpha, D, S, L, U)
        assert bool((mean_e[:, pad] == 0).all()) and bool((alpha_e[:, pad] == 1).all())
        oe, gze = padtrain_ops.embed_rows_raw(om.detach(), D), padtrain_ops.embed_rows_raw(gz, D)
        goe, gpe = torch.empty_like(oe), torch.zeros_like(pe)
        nbytes = check(lib.tnf_flow_forward_train_workspace_bytes(M, M, N, W, S, L))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        check(lib.tnf_flow_forward_train_bwd_f32(oe.data_ptr(), pe.data_ptr(), states.data_ptr(), folds.data_ptr(),
                                                 mean_e.data_ptr(), alpha_e.data_ptr(), gze.data_ptr(), gs.data_ptr(),
                                                 goe.data_ptr(), gpe.data_ptr(), M, M, N, W, S, L, U, pe.shape[1], pe.shape[1],
                                                 ws.data_ptr(), nbytes, tnf._lib.stream_ptr()))
    finally:
        lib.tnf_set_option(tnf._lib.OPT_TRAIN_BWD_FP32, 0)
    assert bool((goe[..., pad] == 0).all())
    # the same launches on the same numbers; sums that float atomics form in any order stand between them
    assert float((goe[..., slots] - om.grad).abs().max()) <= 1e-5 * float(om.grad.abs().max())
    gp = padtrain_ops.gather_params_raw(gpe, (M, P), D, S, L, U)
    assert float((gp - p.grad).abs().max()) <= 1e-5 * float(gp.abs().max())


# ---- 4. train_efn at the width the reference trains ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_train_efn_takes_the_route(tnf, use_graph):
    """notebooks/two_network_arch.ipynb of the reference: NormFlow(D - 1 = 4, "coupling", ..., ToSimplex) under a
    Dirichlet(5) target.  `cde.sample(eta, N, freeze_bn=False)` inside every iteration takes the one-node pair with no change
    of its own; under use_graph the iteration, this pair included, is captured and replayed."""
    from torch_nf_amd.efn import train_efn
    from torch_nf_amd.exponential_families import Dirichlet

    torch.manual_seed(5)
    fam = Dirichlet(5)
    nf = tnf.NormFlow(4, True, "coupling", 1, 1, 15, tnf.ToSimplex(4))
    nf.padded_batch_forward = True
    cde = tnf.ConditionalDensityEstimator(nf, fam.D_eta, [16])
    before = counts(tnf)
    losses, KLs = train_efn(cde, fam, M=8, N=16, num_iters=6, lr=1e-3, seed=3, use_graph=use_graph)
    ran = [a - b for a, b in zip(counts(tnf), before)]
    assert losses.shape == (6,) and KLs.shape == (6,) and np.isfinite(losses).all() and np.isfinite(KLs).all()
    # counted when enqueued: every eager iteration; a graphed run enqueues the warm-up iterations and the captured one only
    # (an iteration that could not be captured would have been finished eagerly: seven)
    assert ran[PB_TRAIN_FWD] == ran[PB_TRAIN_BWD] and ran[PB_FORWARD] == 0, ran
    assert ran[PB_TRAIN_FWD] == (4 if use_graph else 6), ran  # a graphed run: three warm-up iterations and the one capture
