"""The rejection-ABC kernels (include/tnf_abc.h) on the GPU against the numpy restatement (tests/abc_restatement.py).

Error measure: max |got - want| / max(1, max |want|).  A bar is 4 x the error of the float32 twin (the restatement's own
arithmetic in float32) against float64 ON THE SAME INPUTS, computed here, where the test runs:
  E_z over every candidate of the case; E_x over the candidates inside the box and within the case's widest tolerance (the
  values an output can take); the same sets give the denominators of the device's errors.
Chains are compared round by round: round t of the restatement starts from the DEVICE's round t - 1 (its float32 values,
exactly), so every round is checked on identical inputs and no rounding difference is carried from round to round.
A trial is AMBIGUOUS if, in float64, a coordinate lies within 4 E_z max(1, |bound|) of a bound or a statistic within
4 E_x max(1, |x|) of its tolerance edge; a chain leaves the decision comparison from the round in which an ambiguous trial
occurs at or before its accepted trial.  Conditions on the inputs (asserted, not measured): at most 2 % of a case's chains
leave, every round's acceptance rate is at least 2 %, no chain needs more than max_trials / 2 trials.
Starting populations are prior draws that already satisfy round 0's tolerance."""
import numpy as np
import pytest
import torch

import abc_restatement as R

import torch_nf_amd as tnf
from torch_nf_amd import _lib, abc_ops
from torch_nf_amd.lfi import ABC_MCMC, ABC_SMC
from torch_nf_amd.systems import GaussianProposal, Mat

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _count(which):
    return _lib.lib.tnf_abc_launch_count(which)


def _start(d, N, x0, eps0, rng, bound=2.0):
    """N prior draws that satisfy round 0's tolerance."""
    D, out, n = d * (d + 1) // 2, [], 0
    while n < N:
        z = rng.uniform(-bound, bound, (4096, D)).astype(np.float32)
        keep = z[np.all(np.abs(R.stats(z, d) - x0) < eps0, axis=-1)]
        out.append(keep)
        n += len(keep)
    return np.concatenate(out)[:N]


def _case(d, N, T, max_trials, e1, eT, seed, sigma=0.5, offdiag=False):
    rng = np.random.RandomState(seed)
    D = d * (d + 1) // 2
    x0 = np.array([0.0, d / 2.0])
    eps = np.stack([np.linspace(e1[i], eT[i], 4) for i in range(2)], axis=1)[:T]
    Sigma = sigma ** 2 * np.eye(D)
    if offdiag:
        B = rng.normal(0.0, 1.0, (D, D))
        Sigma = sigma ** 2 * (0.6 * np.eye(D) + 0.4 * B @ B.T / D)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(d=d, D=D, N=N, T=T, max_trials=max_trials, x0=f32(x0), eps=f32(eps), L=f32(np.linalg.cholesky(Sigma)),
                lb=f32(-2.0 * np.ones(D)), ub=f32(2.0 * np.ones(D)), z0=_start(d, N, x0, eps[0], rng),
                omega=rng.standard_normal((T, N, max_trials, D)).astype(np.float32))


def _run(c, omega=None, seed=0):
    zs, xs, trials = abc_ops.abc_smc_mat(_dev(c["z0"]), _dev(c["L"]), _dev(np.stack((c["lb"], c["ub"]))), _dev(c["x0"]),
                                         _dev(c["eps"]), c["d"], c["max_trials"], seed,
                                         None if omega is None else _dev(omega))
    torch.cuda.synchronize()
    return zs.cpu().numpy(), xs.cpu().numpy(), trials.cpu().numpy()


def _tolerance_holds(c, xs, trials):
    """the kernel's own comparison, in its own float32: every accepted row satisfies its round's tolerance"""
    dist = np.abs(xs - c["x0"][None, None, :])
    return np.all((dist < c["eps"][:, None, :]).all(-1) == (trials > 0))


def _check_chains(c, zs, xs, trials):
    d, N, T = c["d"], c["N"], c["T"]
    assert zs.shape == (T, N, c["D"]) and xs.shape == (T, N, 2) and trials.shape == (T, N) and trials.dtype == np.int32
    assert (trials > 0).all(), "the cases are built so that every chain finishes"
    rounds = []
    ez_abs = ex_abs = 0.0
    z_max = x_max = 1.0
    for t in range(T):
        mu = c["z0"] if t == 0 else zs[t - 1]
        r64 = R.smc_round(mu, c["L"], c["lb"], c["ub"], c["x0"], c["eps"][t], c["omega"][t], d, np.float64)
        r32 = R.smc_round(mu, c["L"], c["lb"], c["ub"], c["x0"], c["eps"][t], c["omega"][t], d, np.float32)
        near = r64["box"] & np.all(np.abs(r64["x"] - c["x0"]) < c["eps"][0], axis=-1)
        ez_abs = max(ez_abs, float(np.abs(r32["z"] - r64["z"]).max()))
        z_max = max(z_max, float(np.abs(r64["z"]).max()))
        ex_abs = max(ex_abs, float(np.abs(r32["x"] - r64["x"])[near].max()))
        x_max = max(x_max, float(np.abs(r64["x"][near]).max()))
        rounds.append(r64)
    E_z, E_x = ez_abs / z_max, ex_abs / x_max
    left = np.zeros((T, N), dtype=bool)
    rows = np.arange(N)
    err_z = err_x = 0.0
    for t, r in enumerate(rounds):
        assert r["ok"].mean() >= 0.02, "round %d: acceptance rate %.4f" % (t, r["ok"].mean())
        assert 0 < r["trials"].min() and r["trials"].max() <= c["max_trials"] // 2, (t, r["trials"].max())
        bounds = np.stack((c["lb"], c["ub"])).astype(np.float64)
        amb = (np.abs(r["z"][..., None, :] - bounds) <= 4 * E_z * np.maximum(1.0, np.abs(bounds))).any((-1, -2))
        edge = np.abs(np.abs(r["x"] - c["x0"]) - c["eps"][t])
        amb |= (edge <= 4 * E_x * np.maximum(1.0, np.abs(r["x"]))).any(-1)
        upto = np.arange(c["max_trials"])[None, :] < r["trials"][:, None]
        left[t:] |= (amb & upto).any(1)[None, :]
        keep = ~left[t]
        assert np.array_equal(trials[t][keep], r["trials"][keep]), "round %d: accepted trial" % t
        idx = r["trials"] - 1
        err_z = max(err_z, float(np.abs(zs[t] - r["z"][rows, idx])[keep].max(initial=0.0)) / z_max)
        err_x = max(err_x, float(np.abs(xs[t] - r["x"][rows, idx])[keep].max(initial=0.0)) / x_max)
    n_left = int(left[-1].sum())
    print("d=%d N=%d T=%d: E_z %.2e E_x %.2e, device z %.2e x %.2e, %d chains left, sweeps up to %d"
          % (d, N, T, E_z, E_x, err_z, err_x, n_left, (trials.max() + 63) // 64))
    assert n_left <= 0.02 * N, "%d of %d chains left the comparison" % (n_left, N)
    assert err_z <= 4 * E_z and err_x <= 4 * E_x
    assert _tolerance_holds(c, xs, trials)
    return trials


# ---- 1. the stream ---------------------------------------------------------------------------------------------------
def test_stream_matches_the_restatement_and_is_normal():
    seed, Tn, n_i, n_j, D = 0x1234567887654321, 4, 64, 256, 16
    before = _count(_lib.ABC_COUNT_NOISE)
    got = np.stack([abc_ops.abc_noise(seed, t, 0, n_i, 0, n_j, D).cpu().numpy() for t in range(Tn)])
    assert _count(_lib.ABC_COUNT_NOISE) == before + Tn
    want = np.stack([R.noise_block(seed, t, 0, n_i, 0, n_j, D) for t in range(Tn)])
    twin = np.stack([R.noise_block(seed, t, 0, n_i, 0, n_j, D, np.float32) for t in range(Tn)])
    bar, err = 4 * R.rel_err(twin, want), R.rel_err(got, want)
    print("stream: twin %.2e device %.2e" % (bar / 4, err))
    assert err <= bar
    n = got.size
    assert n == 1 << 20
    x = got.astype(np.float64)
    assert abs(x.mean()) <= 5 / np.sqrt(n) and abs(x.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    for axis, name in enumerate(("rounds", "particles", "trials", "coordinates")):
        a, b = np.moveaxis(x, axis, 0)[:-1], np.moveaxis(x, axis, 0)[1:]
        assert abs(float((a * b).mean())) <= 5 / np.sqrt(n), name


def test_stream_subrange_and_ragged_width():
    seed, t, D = 77, 3, 21
    full = abc_ops.abc_noise(seed, t, 0, 12, 0, 70, D)
    sub = abc_ops.abc_noise(seed, t, 5, 7, 60, 10, D)
    assert torch.equal(sub, full[5:12, 60:70])
    want = R.noise_block(seed, t, 0, 12, 0, 70, D)
    bar = 4 * R.rel_err(R.noise_block(seed, t, 0, 12, 0, 70, D, np.float32), want)
    assert R.rel_err(full.cpu().numpy(), want) <= bar
    far = abc_ops.abc_noise(seed, (1 << 31) - 1, (1 << 24) - 2, 2, (1 << 24) - 3, 3, 5).cpu().numpy()  # the counters' ends
    want = R.noise_block(seed, (1 << 31) - 1, (1 << 24) - 2, 2, (1 << 24) - 3, 3, 5)
    assert R.rel_err(far, want) <= bar  # the arithmetic does not depend on the counter: the block's bar serves
    assert tuple(abc_ops.abc_noise(seed, 0, 0, 0, 0, 4, 3).shape) == (0, 4, 3)


# ---- 2. chains with supplied noise --------------------------------------------------------------------------------------
# (d, N, T, max_trials, first and last tolerance of the linear 4-round schedule, off-diagonal Sigma)
CASES = [(2, 256, 4, 256, (4, 2), (1, 0.5), False),
         (2, 1, 1, 256, (4, 2), (1, 0.5), False),
         (3, 63, 4, 1024, (8, 3), (1.5, 0.75), False),
         (3, 64, 1, 1024, (8, 3), (1.5, 0.75), True),
         (4, 65, 4, 512, (15, 4), (4, 1.5), False),
         (5, 64, 4, 1536, (30, 6), (8, 2), False),
         (6, 32, 4, 2048, (60, 8), (20, 3), False)]


@pytest.mark.parametrize("d,N,T,mt,e1,eT,offdiag", CASES, ids=["d%dN%dT%d" % c[:3] for c in CASES])
def test_chains_with_supplied_noise(d, N, T, mt, e1, eT, offdiag):
    c = _case(d, N, T, mt, e1, eT, seed=100 + d, offdiag=offdiag)
    before = _count(_lib.ABC_COUNT_SMC)
    zs, xs, trials = _run(c, c["omega"])
    assert _count(_lib.ABC_COUNT_SMC) == before + 1
    trials = _check_chains(c, zs, xs, trials)
    if d >= 5:  # the accepted trials fall in the first, the second and later 64-trial sweeps
        sweeps = (trials - 1) // 64
        assert (sweeps == 0).any() and (sweeps == 1).any() and (sweeps >= 2).any()


def test_crafted_noise_accepts_exactly_the_zero_row():
    mt = 130  # three sweeps, the last one ragged
    c = _case(2, 4, 1, mt, (4, 2), (1, 0.5), seed=5)
    where = [1, 64, 65, mt]  # 1-based: first, last lane of sweep 1, first lane of sweep 2, last trial
    omega = np.full((1, 4, mt, 3), 100.0, dtype=np.float32)  # z = mu + 50: far outside the box
    for i, j in enumerate(where):
        omega[0, i, j - 1] = 0.0
    zs, xs, trials = _run(c, omega)
    assert trials[0].tolist() == where
    assert np.array_equal(zs[0], c["z0"])  # mu + L 0 = mu, bit for bit
    assert R.rel_err(xs[0], R.stats(c["z0"], 2)) <= 1e-6 and _tolerance_holds(c, xs, trials)
    omega[0, 3, mt - 1] = 100.0  # ... and without its zero row the last chain exhausts the round
    zs, xs, trials = _run(c, omega)
    assert trials[0].tolist() == where[:3] + [0] and np.isnan(zs[0, 3]).all() and np.isnan(xs[0, 3]).all()
    assert np.array_equal(zs[0, :3], c["z0"][:3])


# ---- 3. exhaustion ---------------------------------------------------------------------------------------------------------
def test_exhaustion_stops_a_chain_and_only_that_chain():
    c = _case(2, 8, 4, 128, (4, 2), (4, 2), seed=9)
    c["omega"][1, 4:] = 100.0  # chains 4 .. 7 cannot stay inside the box in round 2 of 4
    zs, xs, trials = _run(c, c["omega"])
    assert (trials[:, :4] > 0).all() and (trials[0] > 0).all() and (trials[1:, 4:] == 0).all()
    assert np.isnan(zs[1:, 4:]).all() and np.isnan(xs[1:, 4:]).all()
    assert np.isfinite(zs[:, :4]).all() and np.isfinite(zs[0]).all() and _tolerance_holds(c, xs, trials)
    want = R.smc_chain(c["z0"], c["L"], c["lb"], c["ub"], c["x0"], c["eps"], 2, 128, c["omega"])[2]
    assert np.array_equal(trials == 0, want == 0)
    c["eps"][1] = 0.0  # an unattainable tolerance (the comparison is strict), in-kernel stream
    zs, xs, trials = _run(c, None, seed=3)
    assert (trials[0] > 0).all() and (trials[1:] == 0).all() and np.isnan(zs[1:]).all() and np.isnan(xs[1:]).all()
    assert np.isfinite(zs[0]).all() and _tolerance_holds(c, xs, trials)


def test_abc_smc_returns_none_when_a_round_is_exhausted():
    mat = Mat(2)
    prop = GaussianProposal(0.25 * np.eye(3), mat.lb, mat.ub)
    eps = np.array([[4.0, 2.0], [0.0, 0.0], [4.0, 2.0], [4.0, 2.0]])
    np.random.seed(4)
    assert ABC_SMC(6, mat, prop, np.array([[0.0, 1.0]]), eps, max_trials=128) is None
    zs, T_xs, trials = ABC_SMC(6, mat, prop, np.array([[0.0, 1.0]]), eps, max_trials=128, return_info=True)
    assert zs is None and T_xs is None and trials.shape == (4, 6) and (trials[1:] == 0).all()
    assert ABC_MCMC(5, mat, prop, np.array([[0.0, 1.0]]), [0.0, 0.0], max_trials=64) is None


# ---- 4. in-kernel stream = supplied stream -------------------------------------------------------------------------------
@pytest.mark.parametrize("d,N,T,mt", [(3, 65, 3, 320), (6, 7, 2, 1000)])
def test_in_kernel_stream_is_the_noise_entry(d, N, T, mt):
    e1 = {3: (8, 3), 6: (60, 8)}[d]
    c = _case(d, N, T, mt, e1, e1, seed=20 + d)
    seed = 0x0BADC0DE12345
    omega = torch.stack([abc_ops.abc_noise(seed, t, 0, N, 0, mt, c["D"]) for t in range(T)])
    fed = _run(c, omega.cpu().numpy(), seed=999)  # the seed is not used when noise is supplied
    own = _run(c, None, seed=seed)
    again = _run(c, None, seed=seed)
    other = _run(c, None, seed=seed + 1)
    assert (own[2] > 0).all()
    for a, b, e in zip(fed, own, again):
        assert np.array_equal(a, b) and np.array_equal(b, e)
    assert not np.array_equal(own[0], other[0]) and not np.array_equal(own[2], other[2])


# ---- 5. GaussianProposal.rvs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,M,shared", [(1, 65, True), (7, 64, False), (21, 130, True)])
def test_propose_with_supplied_noise(D, M, shared):
    rng = np.random.RandomState(D)
    mt = 192
    B = rng.normal(0.0, 1.0, (D, D))
    L = np.linalg.cholesky(0.25 * (0.6 * np.eye(D) + 0.4 * B @ B.T / D)).astype(np.float32)
    lb, ub = -np.ones(D, dtype=np.float32), (1.0 + 0.1 * np.arange(D)).astype(np.float32)
    mu = rng.uniform(-0.9, 0.9, (1 if shared else M, D)).astype(np.float32)
    omega = rng.standard_normal((M, mt, D)).astype(np.float32)
    if D == 21:
        omega[:3] = 100.0  # three draws that never land inside the box ...
        omega[1, mt - 1] = 0.0  # ... but for the last trial of one of them
    before = _count(_lib.ABC_COUNT_PROPOSE)
    z, trials = abc_ops.abc_propose(_dev(mu), _dev(L), _dev(np.stack((lb, ub))), M, mt, 0, _dev(omega))
    assert _count(_lib.ABC_COUNT_PROPOSE) == before + 1
    z, trials = z.cpu().numpy(), trials.cpu().numpy()
    want, want_trials, cand, box = R.propose(mu, L, lb, ub, omega)
    sel = slice(3, None) if D == 21 else slice(None)  # the crafted rows are no measure of the arithmetic
    E_z = R.rel_err(R.candidates(mu, L, omega, np.float32)[sel], cand[sel])
    bounds = np.stack((lb, ub)).astype(np.float64)
    amb = (np.abs(cand[..., None, :] - bounds) <= 4 * E_z * np.maximum(1.0, np.abs(bounds))).any((-1, -2))
    upto = np.arange(mt)[None, :] < np.where(want_trials > 0, want_trials, mt)[:, None]
    keep = ~(amb & upto).any(1)
    assert (~keep).sum() <= 0.02 * M
    assert np.array_equal(trials[keep], want_trials[keep])
    done = keep & (want_trials > 0)
    assert R.rel_err(z[done], want[done], cand[sel]) <= 4 * E_z
    assert np.all((lb < z[done]) & (z[done] < ub))
    if D == 21:
        assert trials[:3].tolist() == [0, mt, 0] and np.isnan(z[0]).all() and np.isnan(z[2]).all()
        assert np.array_equal(z[1], mu[0])


def test_rvs_stays_inside_and_has_the_moments():
    D, M = 3, 1 << 14
    lb, ub = -0.5 * np.ones(D), 0.5 * np.ones(D)
    tight = GaussianProposal(0.25 * np.eye(D), lb, ub)  # one sigma wide: most draws are redrawn
    np.random.seed(0)
    z = tight.rvs(np.array([0.4, -0.4, 0.0]), 4096)
    assert z.shape == (4096, D) and z.dtype == np.float64 and np.all((lb < z) & (z < ub))
    assert tight.rvs(np.zeros(D)).shape == (D,) and tight.rvs(np.zeros((1, D))).shape == (1, D)
    np.random.seed(0)
    assert np.array_equal(tight.rvs(np.array([0.4, -0.4, 0.0]), 4096), z)  # np.random.seed governs the draw
    B = np.array([[1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [-0.3, 0.2, 1.0]])
    Sigma = 0.04 * B @ B.T
    sd = np.sqrt(np.diag(Sigma))
    mu = np.array([0.1, -0.2, 0.05])
    wide = GaussianProposal(Sigma, mu - 5 * sd, mu + 5 * sd)  # a box 10 sigma wide: truncation removes < 2e-6
    z = wide.rvs(mu, M, seed=12)
    assert np.all(np.abs(z.mean(0) - mu) <= 5 * sd / np.sqrt(M))
    C = np.cov(z.T, bias=True)
    assert np.all(np.abs(C - Sigma) <= 5 * np.sqrt((np.outer(sd ** 2, sd ** 2) + Sigma ** 2) / M))


# ---- 6. the drivers -----------------------------------------------------------------------------------------------------------
def _within(system, z, x0, eps):
    """the accepted parameters' statistics, recomputed in float64, are within tolerance plus the float32 margin"""
    x64 = R.stats(z, system.d)
    E = R.rel_err(R.stats(z, system.d, np.float32), x64)
    margin = 4 * E * np.maximum(1.0, np.abs(x64)) + 2.0 ** -22 * (np.abs(x0) + eps)
    return np.all(np.abs(x64 - x0) < eps + margin)


@pytest.mark.parametrize("d", [2, 3])
def test_abc_smc_driver(d):
    mat = Mat(d)
    N, T = 20, 3
    prop = GaussianProposal(np.eye(mat.D), mat.lb, mat.ub)  # wide steps: a prior draw in a corner of the box gets out
    x0 = np.array([[0.0, d / 2.0]])
    e1, eT = {2: ((4, 2), (1, 0.5)), 3: ((8, 3), (1.5, 0.75))}[d]
    all_eps = np.stack([np.linspace(e1[i], eT[i], T) for i in range(2)], axis=1)
    np.random.seed(1)
    before = _count(_lib.ABC_COUNT_SMC)
    zs, T_xs, trials = ABC_SMC(N, mat, prop, x0, all_eps, return_info=True)
    assert _count(_lib.ABC_COUNT_SMC) == before + 1  # all rounds of all particles: one launch
    assert zs.shape == (T + 1, N, mat.D) and T_xs.shape == (T + 1, N, 2) and trials.shape == (T, N)
    assert zs.dtype == np.float64 and (trials > 0).all()
    np.random.seed(1)
    assert np.array_equal(zs[0], mat.prior.rvs(N))
    for t in range(T):
        assert _within(mat, zs[t + 1], x0[0], all_eps[t])
        assert np.all(np.abs(T_xs[t + 1] - mat.simulate(zs[t + 1])) <= 1e-4 * np.maximum(1.0, np.abs(T_xs[t + 1])))
        assert np.all((mat.lb < zs[t + 1]) & (zs[t + 1] < mat.ub))
    np.random.seed(1)
    again = ABC_SMC(N, mat, prop, x0, all_eps)
    assert isinstance(again, np.ndarray) and np.array_equal(again, zs)
    assert not np.array_equal(ABC_SMC(N, mat, prop, x0, all_eps, seed=5)[1:], zs[1:])


@pytest.mark.parametrize("chains", [1, 3])
def test_abc_mcmc_driver(chains):
    mat = Mat(3)
    prop = GaussianProposal(np.eye(mat.D), mat.lb, mat.ub)
    x0, eps, N = np.array([[0.0, 1.5]]), [3.0, 2.0], 40
    np.random.seed(2)
    before = _count(_lib.ABC_COUNT_SMC)
    zs, T_xs = ABC_MCMC(N, mat, prop, x0, eps, chains=chains)
    assert _count(_lib.ABC_COUNT_SMC) == before + 1
    lead = () if chains == 1 else (chains,)
    assert zs.shape == lead + (N, mat.D) and T_xs.shape == lead + (N, 2)
    assert _within(mat, zs.reshape(-1, mat.D), x0[0], np.asarray(eps))
    np.random.seed(2)
    assert np.array_equal(ABC_MCMC(N, mat, prop, x0, eps, chains=chains)[0], zs)


def test_the_scripts_imports_resolve_and_run():
    tnf.install_as_torch_nf()
    ns = {}
    exec("from torch_nf.systems import Mat, GaussianProposal\nfrom torch_nf.lfi import ABC_SMC", ns)
    assert ns["Mat"] is Mat and ns["GaussianProposal"] is GaussianProposal and ns["ABC_SMC"] is ABC_SMC
    mat = ns["Mat"](2)
    np.random.seed(1)
    zs = ns["ABC_SMC"](5, mat, ns["GaussianProposal"](np.eye(3), mat.lb, mat.ub), np.array([[0.0, 1.0]]),
                       np.array([[2.0, 2.0], [1.0, 1.0]]))
    assert zs.shape == (3, 5, 3)
