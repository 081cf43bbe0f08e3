"""A workspace of exactly the queried size is sufficient.

The Python binding hands every entry a grow-only buffer of at least 1 MiB, so no other test runs a kernel against a
workspace of the size its tnf_*_workspace_bytes query returned.  Here `_staging._workspace` is replaced: every `_ws(...)`
call receives a 256-byte aligned view of exactly `nbytes` bytes cut from a larger tensor

    [1 MiB guard | nbytes | guard of max(1 MiB, nbytes)]

whose guards hold a byte pattern before the call and must hold it afterwards.  Each operation runs once with the stock
workspace and once through the fixture; the two results are compared the way that family's own test compares two runs of
one call -- bit for bit where it asserts reproducibility today (reversible backward, wide backward, padded log_prob
pair, MoG, EFN KL), else with that test's tolerance.  The test writes only into memory it allocated: an overrun lands
in a guard and fails an assertion.  Shapes: the smallest at which region sizes stop being multiples of their alignment."""
import numpy as np
import pytest
import torch

from domain_helpers import INV_TOL, LOGP_TOL, SLDF_TOL, ZF_TOL

pytestmark = pytest.mark.gpu

GUARD = 1 << 20
PATTERN = 0xA5


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available()
    return torch_nf_amd


class TightWorkspaces:
    """Stands in for _staging._workspace(nbytes, dev); keeps every buffer it handed out until `check`."""

    def __init__(self):
        self.handed = []

    def __call__(self, nbytes, dev):
        tail = max(GUARD, nbytes)
        buf = torch.full((GUARD + 256 + nbytes + tail,), PATTERN, dtype=torch.uint8, device=dev)
        start = GUARD + (-(buf.data_ptr() + GUARD)) % 256
        view = buf[start:start + nbytes]
        assert view.data_ptr() % 256 == 0 and view.numel() == nbytes
        self.handed.append((buf, start, nbytes))
        return view

    def check(self):
        torch.cuda.synchronize()
        assert self.handed, "the operation asked for no workspace: the case tests nothing"
        for buf, start, nbytes in self.handed:
            assert bool((buf[:start] == PATTERN).all()), "a kernel wrote in front of its %d-byte workspace" % nbytes
            assert bool((buf[start + nbytes:] == PATTERN).all()), "a kernel wrote behind its %d-byte workspace" % nbytes


def both(tnf, monkeypatch, run):
    """run() with the stock workspace, then through the fixture with its guards checked -> (stock, tight)"""
    stock = run()
    torch.cuda.synchronize()
    tight = TightWorkspaces()
    with monkeypatch.context() as m:
        m.setattr(tnf._staging, "_workspace", tight)
        got = run()
        tight.check()
    return stock, got


def same_bits(stock, got):
    assert len(stock) == len(got)
    for a, b in zip(stock, got):
        assert torch.equal(a, b)


def close(stock, got, tols):
    assert len(stock) == len(got) == len(tols)
    for a, b, t in zip(stock, got, tols):
        torch.testing.assert_close(b, a, **t)


def close_to_largest(stock, got, bar):
    """|got - stock| <= bar x the largest entry: the measure of conftest.grad_err"""
    assert float((got.double() - stock.double()).abs().max()) <= bar * float(stock.double().abs().max())


def coupling_flow(tnf, D, S, L, U, Mz, Mp, N, seed):
    """(z, params, bn_mean, bn_alpha) on the GPU for NormFlow(D, 'coupling', S, L, U)"""
    rng = np.random.RandomState(seed)
    P = tnf.NormFlow(D, False, "coupling", S, L, U).D_params
    f = lambda a: torch.tensor(a).float().cuda()  # noqa: E731
    return (f(rng.normal(0, 1, (Mz, N, D))), f(rng.normal(0, 0.1, (Mp, P))), f(rng.normal(0, 0.3, (2 * S, D))),
            f(np.exp(rng.normal(0, 0.2, (2 * S, D)))))


def loss_grads(outs, weights, wrt):
    """gradients of sum_i <outs[i], weights[i]> w.r.t. `wrt`"""
    loss = sum((o * w).sum() for o, w in zip(outs, weights))
    return torch.autograd.grad(loss, wrt)


# ---- whole flow and per-layer chain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Mp", [1, 3])
@pytest.mark.parametrize("D,S,L,U", [(32, 1, 2, 15), (64, 2, 2, 15)])
def test_whole_flow_and_layer_chain(tnf, monkeypatch, D, S, L, U, Mp):
    z, p, mean, alpha = coupling_flow(tnf, D, S, L, U, 3, Mp, 17, 1)
    for fusion in (tnf._lib.FUSE_FLOW, tnf._lib.FUSE_LAYER):
        stock, got = both(tnf, monkeypatch, lambda: tnf.ops.flow_log_prob_raw(z, p, mean, alpha, D, S, L, U, fusion,
                                                                              want_z0=True, want_sld=True))
        close(stock, got, (LOGP_TOL, INV_TOL, INV_TOL))
        stock, got = both(tnf, monkeypatch, lambda: tnf.ops.flow_forward_raw(z, p, mean, alpha, D, S, L, U, fusion))
        close(stock, got, (ZF_TOL, SLDF_TOL))


# ---- training pairs -----------------------------------------------------------------------------------------------------------
def log_prob_training(tnf, fn, z0, p0, mean, alpha, shape, w):
    z, p = z0.clone().requires_grad_(), p0.clone().requires_grad_()
    lp = fn(z, p, mean, alpha, *shape)
    gz, gp = loss_grads([lp], [w], [z, p])
    return lp.detach(), gz, gp


def test_layer_pair_training(tnf, monkeypatch):
    D, S, L, U, M, N = 32, 2, 2, 15, 3, 33
    z0, p0, mean, alpha = coupling_flow(tnf, D, S, L, U, M, M, N, 2)
    w = torch.tensor(np.random.RandomState(3).normal(0, 1, (M, N))).float().cuda() / N
    fn = lambda *a: tnf.ops.flow_log_prob_train(*a, reversible=False)  # noqa: E731
    stock, got = both(tnf, monkeypatch, lambda: log_prob_training(tnf, fn, z0, p0, mean, alpha, (D, S, L, U), w))
    # test_gpu_grad.test_flow_level_training_pair: the layer backward adds with float atomics
    close(stock, got, (dict(rtol=1e-5, atol=1e-4), dict(rtol=2e-4, atol=2e-6), dict(rtol=5e-4, atol=5e-5)))


@pytest.mark.parametrize("Mp", [1, 3])
def test_reversible_training(tnf, monkeypatch, Mp):
    D, S, L, U, M, N = 64, 1, 2, 15, 3, 17
    z0, p0, mean, alpha = coupling_flow(tnf, D, S, L, U, M, Mp, N, 4)
    w = torch.tensor(np.random.RandomState(5).normal(0, 1, (M, N))).float().cuda() / N
    if Mp == 1:
        assert tnf.ops.flow_train_rev_supported(M, Mp, N, D, S, L, U)
        fn = lambda *a: tnf.ops.flow_log_prob_train(*a, reversible=True)  # noqa: E731
    else:
        # a row per context with fewer than 32 samples: flow_log_prob_train would hand this layout to the layer pair
        # (a choice of speed); the reversible entries themselves take it, and their workspace is what is tested here
        assert tnf._lib.lib.tnf_flow_train_rev_supported(D, S, L, U) == 1
        fn = tnf.ops._FlowLogProbRevFn.apply
    stock, got = both(tnf, monkeypatch, lambda: log_prob_training(tnf, fn, z0, p0, mean, alpha, (D, S, L, U), w))
    same_bits(stock, got)  # test_gpu_grad: fixed-point accumulators, sums in block order


# ---- batch statistics ---------------------------------------------------------------------------------------------------------
# two runs differ by the order of the double-precision atomics behind the moments: the bars test_gpu_grad._one_node_body
# and test_gpu_padded_batch put between two routes to the same numbers
STATS_TOLS = (dict(rtol=2e-5, atol=2e-5), dict(rtol=1e-6, atol=2e-4), dict(rtol=2e-5, atol=2e-5), dict(rtol=2e-5, atol=2e-5))


def sampling_training(forward_train, om0, p0, shape, wz, ws):
    om, p = om0.clone().requires_grad_(), p0.clone().requires_grad_()
    z, sld, mean, alpha = forward_train(om, p, *shape, 1e-5)
    g_om, g_p = loss_grads([z, sld], [wz, ws], [om, p])
    return z.detach(), sld.detach(), mean.detach(), alpha.detach(), g_om, g_p


def check_sampling_training(stock, got):
    close(stock[:4], got[:4], STATS_TOLS)
    for a, b in zip(stock[4:], got[4:]):
        torch.testing.assert_close(b, a, rtol=1e-3, atol=1e-4 * float(a.abs().max()))


def test_batch_statistics(tnf, monkeypatch):
    D, S, L, U, M, N = 32, 2, 2, 15, 3, 33
    om, p, _, _ = coupling_flow(tnf, D, S, L, U, M, M, N, 6)
    stock, got = both(tnf, monkeypatch, lambda: tnf.ops.flow_forward_batch_raw(om, p, D, S, L, U, 1e-5))
    close(stock, got, STATS_TOLS)
    rng = np.random.RandomState(7)
    wz, ws = (torch.tensor(rng.normal(0, 1, s)).float().cuda() / N for s in ((M, N, D), (M, N)))
    stock, got = both(tnf, monkeypatch,
                      lambda: sampling_training(tnf.ops.flow_forward_train, om, p, (D, S, L, U), wz, ws))
    check_sampling_training(stock, got)


# ---- padded -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [5, 47])
def test_padded(tnf, monkeypatch, D):
    S, L, U, M, N = 2, 2, 15, 3, 33
    z, p, mean, alpha = coupling_flow(tnf, D, S, L, U, M, M, N, 8 + D)
    rng = np.random.RandomState(9)
    w, wz, ws = (torch.tensor(rng.normal(0, 1, s)).float().cuda() / N for s in ((M, N), (M, N, D), (M, N)))
    stock, got = both(tnf, monkeypatch, lambda: tnf.ops.flow_padded_log_prob_raw(z, p, mean, alpha, D, S, L, U, want_z0=True,
                                                                                want_sld=True))
    same_bits(stock, got)
    fn = tnf.padtrain_ops.flow_padded_log_prob_train
    stock, got = both(tnf, monkeypatch, lambda: log_prob_training(tnf, fn, z, p, mean, alpha, (D, S, L, U), w))
    same_bits(stock, got)  # test_gpu_padded_train: the reversible pair at the padded width
    stock, got = both(tnf, monkeypatch, lambda: tnf.padbatch_ops.flow_padded_forward_batch_raw(z, p, D, S, L, U, 1e-5))
    close(stock, got, STATS_TOLS)
    stock, got = both(tnf, monkeypatch,
                      lambda: sampling_training(tnf.padbatch_ops.flow_padded_forward_train, z, p, (D, S, L, U), wz, ws))
    check_sampling_training(stock, got)


# ---- conditional flow ---------------------------------------------------------------------------------------------------------
def test_conditional_flow(tnf, monkeypatch):
    D, S, L, U, H, M = 32, 1, 2, 15, 50, 33  # H = 50: the wrapper pads the conditioner's width to 64
    rng = np.random.RandomState(10)
    P = tnf.NormFlow(D, True, "coupling", S, L, U).D_params
    f = lambda a: torch.tensor(a).float().cuda()  # noqa: E731
    z, h, wt, b = f(rng.normal(0, 1, (M, D))), f(rng.normal(0, 1, (M, H))), f(rng.normal(0, 0.1 / np.sqrt(H), (P, H))), \
        f(rng.normal(0, 0.1, (P,)))
    mean, alpha, w = f(rng.normal(0, 0.3, (2 * S, D))), f(np.exp(rng.normal(0, 0.2, (2 * S, D)))), f(rng.normal(0, 1, (M,)))
    stock, got = both(tnf, monkeypatch, lambda: tnf.ops.cond_flow_log_prob_raw(z, h, wt, b, mean, alpha, D, S, L, U,
                                                                              want_z0=True, want_sld=True))
    close(stock, got, (LOGP_TOL, INV_TOL, INV_TOL))

    def train():
        leaves = [t.clone().requires_grad_() for t in (z, h, wt, b)]
        lp = tnf.ops.cond_flow_log_prob_train(*leaves, mean, alpha, D, S, L, U)
        return (lp.detach(),) + loss_grads([lp], [w], leaves)

    stock, got = both(tnf, monkeypatch, train)
    torch.testing.assert_close(got[0], stock[0], rtol=1e-5, atol=1e-5)
    close_to_largest(stock[1], got[1], 4e-6)  # test_gpu_cond: d z
    for a, b_ in zip(stock[2:], got[2:]):
        close_to_largest(a, b_, 1.1e-5)  # test_gpu_cond: d param_net


# ---- AR flow ------------------------------------------------------------------------------------------------------------------
def test_ar_flow(tnf, monkeypatch):
    D, L, U, Mp, N = 5, 2, 15, 3, 17
    np.random.seed(11)  # the masks' degree vectors
    nf = tnf.NormFlow(D, True, "AR", 1, L, U)
    masks = nf.bijectors[0]._masks_flat
    rng = np.random.RandomState(12)
    f = lambda a: torch.tensor(a).float().cuda()  # noqa: E731
    z, p0 = f(rng.uniform(-1.5, 1.5, (Mp, N, D))), f(rng.normal(0, 0.2, (Mp, nf.D_params)))
    mean, alpha, w = f(rng.normal(0, 0.3, D)), f(np.exp(rng.normal(0, 0.2, D))), f(rng.uniform(0.2, 1.0, (Mp, N))) / N
    stock, got = both(tnf, monkeypatch, lambda: tnf.ops.ar_flow_log_prob_raw(z, p0, masks, mean, alpha, D, L, U, want_z0=True,
                                                                            want_sld=True))
    close(stock, got, (LOGP_TOL, INV_TOL, INV_TOL))

    def train():
        p = p0.clone().requires_grad_()
        lp = tnf.ops.ar_flow_log_prob_train(z, p, masks, mean, alpha, None, D, L, U)
        return (lp.detach(),) + loss_grads([lp], [w], [p])

    stock, got = both(tnf, monkeypatch, train)
    torch.testing.assert_close(got[0], stock[0], **LOGP_TOL)
    # test_gpu_maf: the bar between the one-kernel backward and the per-bijector route
    torch.testing.assert_close(got[1], stock[1], rtol=2e-4, atol=2e-5 * float(stock[1].abs().max()))


# ---- wide backward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["coupling", "maf"])
def test_wide_backward(tnf, monkeypatch, kind):
    D, L, N = 64, 2, 100
    if kind == "coupling":
        layer, fam = tnf.RealNVP(D, L, 20, transform_upper=True), tnf._lib.DIAG_BWD_WIDE
    else:
        np.random.seed(5)
        layer, fam = tnf.MAF(D, L, 64), tnf._lib.DIAG_MAF_BWD_MFMA
    rng = np.random.RandomState(13)
    f = lambda a: torch.tensor(a).float().cuda()  # noqa: E731
    p0, z0 = f(rng.normal(0, 0.05, (1, layer.count_num_params()))), f(rng.normal(0, 1, (1, N, D)))
    wz, wl = f(rng.normal(0, 1, (1, N, D))), f(rng.normal(0, 1, (1, N)))

    def run():
        p, z = p0.clone().requires_grad_(), z0.clone().requires_grad_()
        return loss_grads(layer.inverse_and_log_det(z, p), [wz, wl], [p, z])

    before = tnf._lib.lib.tnf_diag_launch_count(fam)
    stock, got = both(tnf, monkeypatch, run)
    assert tnf._lib.lib.tnf_diag_launch_count(fam) == before + 2  # the two-pass MFMA backward, both times
    same_bits(stock, got)  # test_gpu_grad: no atomics, partial rows added in order


# ---- MoG, EFN -----------------------------------------------------------------------------------------------------------------
def test_mog_backward_shared_row(tnf, monkeypatch):
    from test_gpu_mog import make_case

    D, K, N = 3, 2, 300
    z0, p0, lb, ub = make_case(D, K, (1, 1, N), False, seed=1)
    assert lb is None and ub is None
    g = torch.tensor(np.random.RandomState(14).normal(0, 1, (1, N))).float().cuda()

    def run():
        z, p = z0.cuda().requires_grad_(), p0.cuda().requires_grad_()
        return loss_grads([tnf.mog_ops.mog_log_prob(z, p, D, K)], [g], [z, p])

    same_bits(*both(tnf, monkeypatch, run))  # test_gpu_mog: bit-reproducible


def test_efn_kl(tnf, monkeypatch):
    from test_gpu_efn import _kl_case, dev

    fam, eta, z, lq, _, _ = _kl_case("mvn", 5, 3, 130)
    zd, lqd, ed = dev(z), dev(lq), dev(eta)
    same_bits(*both(tnf, monkeypatch, lambda: (fam.KL_device(zd, lqd, ed),)))  # test_gpu_efn: reproducible bit for bit
