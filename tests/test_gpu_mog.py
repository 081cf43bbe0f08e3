"""MoG on the GPU against float64: tests/mog_restatement.py (pinned to the reference by tests/test_mog_host.py) is the
oracle.  Error measure: max |got - want| / max(1, max |want|) per case.  Bars are not constants: a bar is 4 x the
largest error, over the test's own cases, of the float32 CPU restatement against float64 on the same inputs -- the
reference's own float32 noise, computed where the test runs.  Gradients go through conftest.grad_err with the same rule.
Every K > 1 case asserts that no oracle value is below -20 before it compares: z is drawn near the component means, so
a badly drawn case fails and cannot pass on the flat floor log(1e-12)."""
import copy
import re

import numpy as np
import pytest
import torch

from conftest import grad_err, load_golden
import mog_restatement as R

import torch_nf_amd as tnf
from torch_nf_amd import _lib, ops
from torch_nf_amd.density_estimator import MoG

pytestmark = pytest.mark.gpu

SHAPES = [(D, K) for D in (2, 3, 5, 8, 16) for K in (1, 2, 5)] + [(17, 1), (33, 1)]
LAYOUTS = [(1, 1, 1), (1, 1, 127), (1, 1, 128), (1, 1, 129), (3, 3, 1), (63, 63, 1), (64, 64, 1), (65, 65, 1), (5, 5, 31),
           (5, 5, 65), (5, 1, 33), (1, 5, 33)]  # (M_z, M_p, N): the tile edges of both layouts, both broadcasts
GRAD_CASES = [(5, 5, (64, 64, 1), False), (5, 5, (65, 65, 1), True), (3, 2, (5, 5, 31), True), (8, 2, (5, 5, 65), False),
              (16, 5, (1, 1, 129), True), (5, 1, (1, 1, 129), False), (2, 1, (3, 3, 1), True), (5, 2, (5, 1, 33), False),
              (5, 2, (1, 5, 33), True), (16, 1, (63, 63, 1), False), (17, 1, (3, 3, 1), False), (17, 1, (1, 1, 129), True),
              # the generic backward beyond what LDS could hold: any D, any K
              (36, 1, (3, 3, 1), True), (36, 1, (1, 1, 129), False), (40, 1, (5, 5, 3), False),
              (16, 30, (1, 1, 70), True), (16, 30, (5, 5, 3), False)]  # K = 30: a prepared row beyond the fused kernels'


def bounds_for(D, rng):
    """Multiples of 1/8 (exact in float32), half-widths m around 1: wide boxes only lower the density (Sigma_det has
    the factor prod m_i), and at D = 16 the oracle must stay off the floor."""
    return -np.round(8 * rng.uniform(0.5, 1.5, D)) / 8.0, np.round(8 * rng.uniform(0.75, 2.0, D)) / 8.0


def make_case(D, K, layout, bounded, seed=0):
    """float32 (z, params) and bounds: params ~ 0.5 N(0, 1) (one row per context; for a z shared by several contexts the
    rows are one row + 0.05 N(0, 1), so that the one z is near a mean of each), the factor's entries halved and 0.5 added to every u_ii (sharper
    components: at D = 16 a unit Gaussian's own log-density is -14.7 at its mean); z = a component mean + 0.25 N(0, 1)."""
    Mz, Mp, N = layout
    rng = np.random.RandomState(seed + 1000 * D + 100 * K + 7 * Mz + 3 * Mp + N + int(bounded))
    lb, ub = bounds_for(D, rng) if bounded else (None, None)
    P = K * (1 + D + D * (D + 1) // 2)
    if Mz < Mp:
        params = 0.5 * rng.normal(0, 1, (1, P)) + 0.05 * rng.normal(0, 1, (Mp, P))
    else:
        params = 0.5 * rng.normal(0, 1, (Mp, P))
    T = D * (D + 1) // 2
    diag = np.array([K + K * D + k * T + i * D - i * (i - 1) // 2 for k in range(K) for i in range(D)])
    params[:, K + K * D:] *= 0.5
    params[:, diag] += 0.5
    params = params.astype(np.float32)
    _, mu, _, _ = R.mog_params(torch.tensor(params.astype(np.float64)), D, K, lb, ub)
    mu = mu.numpy()
    comp = rng.randint(0, K, (Mz, N))
    rows = np.arange(Mz)[:, None] if Mp == Mz else np.zeros((Mz, 1), dtype=int)
    z = (mu[rows, comp] + 0.25 * rng.normal(0, 1, (Mz, N, D))).astype(np.float32)
    return torch.tensor(z), torch.tensor(params), lb, ub


def err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


def oracle(z, params, D, K, lb, ub):
    lp64 = R.log_prob(z.double(), params.double(), D, K, lb, ub)
    if K > 1:
        assert float(lp64.min()) > -20.0, "a badly drawn case: the oracle touches the EPS floor (%g)" % float(lp64.min())
    return lp64


def sweep_cases():
    for D, K in SHAPES:
        for layout in LAYOUTS:
            for bounded in (False, True):
                yield D, K, layout, bounded


@pytest.fixture(scope="module")
def lp_bar():
    """4 x the largest float32-restatement error over the whole sweep, and the oracle of every case (computed once)."""
    worst, ref = 0.0, {}
    for D, K, layout, bounded in sweep_cases():
        z, p, lb, ub = make_case(D, K, layout, bounded)
        lp64 = oracle(z, p, D, K, lb, ub)
        worst = max(worst, err(R.log_prob(z, p, D, K, lb, ub), lp64))
        ref[(D, K, layout, bounded)] = lp64
    print("float32 restatement noise over the sweep: %.3e" % worst)
    assert 1e-9 < worst < 1e-5
    return 4.0 * worst, ref


def _bounds_t(lb, ub):
    return None if lb is None else torch.tensor(np.stack([lb, ub]), dtype=torch.float32)


def _count(which):
    return _lib.lib.tnf_mog_launch_count(which)


# ---- golden parity ---------------------------------------------------------------------------------------------------------
def test_golden_parity():
    gold = load_golden("mog")
    keys = sorted({re.match(r"(d\d+k\d+[ub]_|floor_)", n).group(1) for n in gold})
    assert len(keys) == 13
    noise = max(err(torch.tensor(gold[k + "lp32"]), torch.tensor(gold[k + "lp64"])) for k in keys if k != "floor_")
    gnoise = 0.0
    runs = []
    for k in keys:
        D, K = (16, 2) if k == "floor_" else tuple(int(v) for v in re.match(r"d(\d+)k(\d+)", k).groups())
        lb, ub = gold.get(k + "lb"), gold.get(k + "ub")
        mog = MoG(D, True, K, lb, ub)
        p = torch.tensor(gold[k + "params"]).cuda().requires_grad_()
        lp = mog.log_prob(torch.tensor(gold[k + "z"]).cuda(), p)
        (gp,) = torch.autograd.grad((lp * torch.tensor(gold[k + "g_lp"]).float().cuda()).sum(), p)
        assert bool(torch.isfinite(gp).all())
        if k == "floor_":
            assert float((lp.cpu().double() - torch.tensor(gold[k + "lp64"])).abs().max()) <= 1e-5
            continue
        p32 = torch.tensor(gold[k + "params"], requires_grad=True)
        lp32 = R.log_prob(torch.tensor(gold[k + "z"]), p32, D, K, lb, ub)
        (g32,) = torch.autograd.grad((lp32 * torch.tensor(gold[k + "g_lp"]).float()).sum(), p32)
        want = torch.tensor(gold[k + "g_params"])
        gnoise = max(gnoise, float((g32.double() - want).abs().max() / want.abs().max()))
        runs.append((k, lp, gp, want))
    for k, lp, gp, want in runs:
        e = err(lp, torch.tensor(gold[k + "lp64"]))
        print("golden %s lp err %.3e (bar %.3e)" % (k, e, 4 * noise))
        assert e <= 4 * noise, (k, e, noise)
        grad_err("mog_golden_gparams", gp, want, 4 * gnoise)


# ---- the shape sweep -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K", SHAPES)
def test_log_prob_sweep(lp_bar, D, K):
    bar, ref = lp_bar
    fused = _lib.lib.tnf_mog_supported(D, K) == 1
    assert fused == (D <= 16)
    worst = 0.0
    for layout in LAYOUTS:
        for bounded in (False, True):
            z, p, lb, ub = make_case(D, K, layout, bounded)
            mog = MoG(D, True, K, lb, ub)
            before = _count(_lib.MOG_COUNT_LOGPROB)
            with torch.no_grad():
                lp = mog.log_prob(z.cuda(), p.cuda())
            assert _count(_lib.MOG_COUNT_LOGPROB) == before + (1 if fused else 0)  # the fused kernel, or not it
            assert lp.dtype == torch.float32 and tuple(lp.shape) == (max(layout[0], layout[1]), layout[2])
            e = err(lp, ref[(D, K, layout, bounded)])
            worst = max(worst, e)
            assert e <= bar, (D, K, layout, bounded, e, bar)
            if fused and layout in ((1, 1, 129), (65, 65, 1), (5, 5, 31), (1, 5, 33)):
                with _lib.option_set(_lib.OPT_FORCE_GENERIC, 1):
                    before = _count(_lib.MOG_COUNT_LOGPROB)
                    lpg = ops.mog_log_prob_raw(z.cuda(), p.cuda(), D, K, _bounds_t(lb, ub))
                    assert _count(_lib.MOG_COUNT_LOGPROB) == before
                assert err(lpg, ref[(D, K, layout, bounded)]) <= bar
    print("D=%d K=%d worst lp err %.3e (bar %.3e)" % (D, K, worst, bar))


def test_dtype_refused():
    mog = MoG(3, True, 2)
    with pytest.raises(TypeError, match="float32 only"):
        mog.log_prob(torch.zeros(1, 2, 3, dtype=torch.float64).cuda(), torch.zeros(1, mog.D_params, dtype=torch.float64).cuda())


# ---- backward ----------------------------------------------------------------------------------------------------------------
def _grads64(z, p, g, D, K, lb, ub, dtype):
    zz, pp = z.to(dtype).requires_grad_(), p.to(dtype).requires_grad_()
    lp = R.log_prob(zz, pp, D, K, lb, ub)
    return torch.autograd.grad((lp * g.to(dtype)).sum(), [zz, pp])


@pytest.fixture(scope="module")
def grad_bars():
    nz = npar = 0.0
    ref = {}
    for i, (D, K, layout, bounded) in enumerate(GRAD_CASES):
        z, p, lb, ub = make_case(D, K, layout, bounded, seed=1)
        oracle(z, p, D, K, lb, ub)
        g = torch.tensor(np.random.RandomState(i).normal(0, 1, (max(layout[:2]), layout[2])))
        gz64, gp64 = _grads64(z, p, g, D, K, lb, ub, torch.float64)
        gz32, gp32 = _grads64(z, p, g, D, K, lb, ub, torch.float32)
        nz = max(nz, float((gz32.double() - gz64).abs().max() / gz64.abs().max()))
        npar = max(npar, float((gp32.double() - gp64).abs().max() / gp64.abs().max()))
        ref[i] = (g, gz64, gp64)
    print("float32 restatement gradient noise: g_z %.3e g_params %.3e" % (nz, npar))
    return 4.0 * nz, 4.0 * npar, ref


@pytest.mark.parametrize("i", range(len(GRAD_CASES)))
def test_backward(grad_bars, i):
    bar_z, bar_p, ref = grad_bars
    D, K, layout, bounded = GRAD_CASES[i]
    z, p, lb, ub = make_case(D, K, layout, bounded, seed=1)
    g, gz64, gp64 = ref[i]
    mog = MoG(D, True, K, lb, ub)
    outs = []
    for _ in range(2):
        zc, pc = z.cuda().requires_grad_(), p.cuda().requires_grad_()
        before = _count(_lib.MOG_COUNT_LOGPROB_BWD)
        gz, gp = torch.autograd.grad((mog.log_prob(zc, pc) * g.float().cuda()).sum(), [zc, pc])
        assert _count(_lib.MOG_COUNT_LOGPROB_BWD) == before + _lib.lib.tnf_mog_supported(D, K)
        outs.append((gz, gp))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])  # bit-reproducible
    assert gz.shape == z.shape and gp.shape == p.shape
    if K == 1:
        assert float(gp[:, 0].abs().max()) == 0.0  # alpha is ignored
    grad_err("mog_gz", gz, gz64, bar_z)
    grad_err("mog_gparams", gp, gp64, bar_p)
    # z a constant: the g_z = NULL path gives the same parameter gradient, bit for bit
    pc = p.cuda().requires_grad_()
    (gp2,) = torch.autograd.grad((mog.log_prob(z.cuda(), pc) * g.float().cuda()).sum(), [pc])
    assert torch.equal(gp2, outs[0][1])
    # params as a slice of a wider tensor (the ld_params path)
    wide = torch.zeros(p.shape[0], p.shape[1] + 5).cuda()
    wide[:, 3:3 + p.shape[1]] = p.cuda()
    wide.requires_grad_()
    (gw,) = torch.autograd.grad((mog.log_prob(z.cuda(), wide[:, 3:3 + p.shape[1]]) * g.float().cuda()).sum(), [wide])
    assert torch.equal(gw[:, 3:3 + p.shape[1]], outs[0][1]) and float(gw[:, :3].abs().max()) == 0.0
    if _lib.lib.tnf_mog_supported(D, K) and i % 3 == 0:
        with _lib.option_set(_lib.OPT_FORCE_GENERIC, 1):
            zc, pc = z.cuda().requires_grad_(), p.cuda().requires_grad_()
            before = _count(_lib.MOG_COUNT_LOGPROB_BWD)
            gzg, gpg = torch.autograd.grad((mog.log_prob(zc, pc) * g.float().cuda()).sum(), [zc, pc])
            assert _count(_lib.MOG_COUNT_LOGPROB_BWD) == before
        grad_err("mog_gz_generic", gzg, gz64, bar_z)
        grad_err("mog_gparams_generic", gpg, gp64, bar_p)


def test_backward_many_tiles_reduces_in_order():
    """One shared row over 40 tiles in several chunks: the partial rows and their ordered sum."""
    D, K = 5, 3
    z, p, lb, ub = make_case(D, K, (1, 1, 5000), True, seed=2)
    oracle(z, p, D, K, lb, ub)
    g = torch.tensor(np.random.RandomState(5).normal(0, 1, (1, 5000)))
    _, gp64 = _grads64(z, p, g, D, K, lb, ub, torch.float64)
    _, gp32 = _grads64(z, p, g, D, K, lb, ub, torch.float32)
    noise = float((gp32.double() - gp64).abs().max() / gp64.abs().max())
    assert _lib.lib.tnf_mog_bwd_workspace_bytes(1, 1, 5000, D, K) == 40 * p.shape[1] * 4
    mog = MoG(D, True, K, lb, ub)
    outs = []
    for _ in range(2):
        pc = p.cuda().requires_grad_()
        outs.append(torch.autograd.grad((mog.log_prob(z.cuda(), pc) * g.float().cuda()).sum(), [pc])[0])
    assert torch.equal(outs[0], outs[1])
    grad_err("mog_gparams_long", outs[0], gp64, 4 * noise)


# ---- sampling ----------------------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(3, 7, 5, 4, True), (1, 200, 8, 2, False), (4, 70, 2, 3, True), (70, 1, 16, 5, False), (2, 9, 5, 1, True),
                (3, 5, 17, 1, False)]


def test_sampling_with_injected_draws():
    drawn, worst_ref = [], 0.0
    for M, N, D, K, bounded in SAMPLE_CASES:
        rng = np.random.RandomState(40 + D + K)
        lb, ub = bounds_for(D, rng) if bounded else (None, None)
        p = torch.tensor(0.5 * rng.normal(0, 1, (M, K * (1 + D + D * (D + 1) // 2)))).float()
        u = torch.tensor(rng.uniform(0, 1, (M, N))).float()
        e1, e2 = torch.tensor(rng.normal(0, 1, (2, M, N, D))).float()
        # any u closer than 1e-4 to a cumulative-alpha boundary is redrawn: there float32 and float64 may pick
        # different components, which is no error of the kernel
        for _ in range(20):
            _, _, gap = R.sample_map(p.double(), u.double(), e1.double(), e2.double(), D, K, lb, ub)
            close = gap < 1e-4
            if not bool(close.any()):
                break
            u[close] = torch.tensor(rng.uniform(0, 1, int(close.sum()))).float()
        assert not bool(close.any())
        z64, k64, _ = R.sample_map(p.double(), u.double(), e1.double(), e2.double(), D, K, lb, ub)
        z32, k32, _ = R.sample_map(p, u, e1, e2, D, K, lb, ub)
        assert torch.equal(k32, k64)
        worst_ref = max(worst_ref, err(z32, z64))
        drawn.append((M, N, D, K, lb, ub, p, u, e1, e2, z64, k64))
    assert worst_ref > 1e-9
    for M, N, D, K, lb, ub, p, u, e1, e2, z64, k64 in drawn:
        mog = MoG(D, True, K, lb, ub)
        before = _count(_lib.MOG_COUNT_SAMPLE)
        z, lq = mog._forward_from(u.cuda(), e1.cuda(), e2.cuda(), p.cuda())
        assert _count(_lib.MOG_COUNT_SAMPLE) == before + (1 if D <= 16 else 0)
        assert z.dtype == lq.dtype == torch.float32 and tuple(z.shape) == (M, N, D) and tuple(lq.shape) == (M, N)
        if K > 1:
            assert len(set(k64.flatten().tolist())) > 1  # more than one component was drawn
        e = err(z, z64)
        print("sample M=%d N=%d D=%d K=%d err %.3e (bar %.3e)" % (M, N, D, K, e, 4 * worst_ref))
        assert e <= 4 * worst_ref
        with torch.no_grad():
            assert torch.equal(lq, mog.log_prob(z, p.cuda()))  # log_q is this class's log_prob of the samples, bit for bit


def test_forward_and_sample_are_reproducible():
    mog = MoG(5, False, 3)
    np.random.seed(11)
    z1, q1 = mog(N=50)
    np.random.seed(11)
    z2, q2 = mog(N=50)
    assert torch.equal(z1, z2) and torch.equal(q1, q2) and tuple(z1.shape) == (1, 50, 5) and z1.dtype == torch.float32
    assert not z1.requires_grad and bool(torch.isfinite(q1).all())
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    a = mog.sample(64, generator=gen)
    gen.manual_seed(3)
    b = mog.sample(64, generator=gen)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and tuple(a[0].shape) == (1, 64, 5)
    # log_q is the density of the samples
    with torch.no_grad():
        assert torch.equal(a[1], mog.log_prob(a[0]))


# ---- ConditionalDensityEstimator, LFI, graphs --------------------------------------------------------------------------------
def test_cde_with_mog():
    torch.manual_seed(4)
    D, K, Dx, M = 3, 2, 4, 70
    mog = MoG(D, True, K)
    cde = tnf.ConditionalDensityEstimator(mog, Dx, [16])
    x = torch.randn(M, Dx)
    net64 = copy.deepcopy(cde.param_net).cpu().double()
    with torch.no_grad():
        _, mu, _, _ = R.mog_params(net64(x.double()), D, K)
    z = (mu[:, 0, :] + 0.3 * torch.randn(M, D, dtype=torch.float64)).float()

    def ref(dtype):
        net = copy.deepcopy(cde.param_net).cpu().to(dtype)
        lp = R.log_prob(z.to(dtype)[:, None, :], net(x.to(dtype)), D, K)
        return lp, torch.autograd.grad(lp.mean(), list(net.parameters()))

    lp64, g64 = ref(torch.float64)
    assert float(lp64.min()) > -20.0
    lp32, g32 = ref(torch.float32)
    lp = cde.log_prob(z.cuda()[:, None, :], x.cuda())
    assert tuple(lp.shape) == (M, 1)
    assert err(lp, lp64) <= 4 * err(lp32, lp64)
    grads = torch.autograd.grad(lp.mean(), list(cde.param_net.parameters()))
    for got, w32, w64 in zip(grads, g32, g64):
        noise = float((w32.double() - w64).abs().max() / w64.abs().max())
        grad_err("mog_cde_net", got, w64, 4 * noise)
    np.random.seed(0)
    with torch.no_grad():
        zs, lq = cde(x.cuda(), N=5)
        zd, lqd = cde.sample(x.cuda(), N=5)
    for a, b in ((zs, lq), (zd, lqd)):
        assert tuple(a.shape) == (M, 5, D) and tuple(b.shape) == (M, 5) and a.dtype == b.dtype == torch.float32
        assert a.is_cuda and bool(torch.isfinite(b).all())


def test_train_apt_runs_with_a_mog_cde():
    from torch_nf_amd.lfi import train_APT
    from torch_nf_amd.systems import Mat

    np.random.seed(6)
    torch.manual_seed(6)
    mat = Mat(2, noise=0.05)
    cde = tnf.ConditionalDensityEstimator(MoG(mat.D, True, 3), 2, [16])
    cde, losses, zs, lqs, _ = train_APT(cde, mat, np.array([[0.0, 1.0]]), M=64, M_atom=8, R=2, num_iters=8, lr=1e-3,
                                        num_sims=256)  # use_graph at its default: each round's step replays as a graph
    assert losses.shape == (16,) and np.isfinite(losses).all()
    assert zs[0].shape == (64, mat.D) and np.isfinite(lqs[-1]).all()


@pytest.mark.parametrize("bounded", [False, True])
def test_graphed_step_replays_the_eager_loss(bounded):
    from torch_nf_amd.graphs import GraphedStep

    D, K, Dx, M = 5, 5, 3, 256
    lb, ub = (-2.0 * np.ones(D), 3.0 * np.ones(D)) if bounded else (None, None)
    rng = np.random.RandomState(8)
    x = torch.tensor(rng.normal(0, 1, (M, Dx))).float().cuda()
    z = torch.tensor(rng.normal(0, 1, (M, 1, D))).float().cuda()
    torch.manual_seed(8)
    cde0 = tnf.ConditionalDensityEstimator(MoG(D, True, K, lb, ub), Dx, [16])
    res = {}
    for mode in ("eager", "graph"):
        cde = copy.deepcopy(cde0)
        opt = torch.optim.Adam(cde.param_net.parameters(), lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = -cde.log_prob(z, x).mean()
            loss.backward()
            opt.step()
            return loss.detach()

        if mode == "eager":
            res[mode] = np.array([step().item() for _ in range(8)])
        else:
            gs = GraphedStep(step, warmup=3)
            res[mode] = np.array([w.item() for w in gs.warmup_outputs] + [gs().item() for _ in range(5)])
    assert np.isfinite(res["eager"]).all() and res["eager"][-1] < res["eager"][0]
    np.testing.assert_allclose(res["graph"], res["eager"], rtol=1e-5)
