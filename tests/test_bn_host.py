"""The host half of the Affine / BatchNorm / base-density sweep (tests/test_gpu_bn_domain.py), no GPU: what licenses its
references, its bars and its case names.

The sweep compares every kernel with the float64 restatements of tests/bn_restatement.py under bars of 4 x the float32
reference's own error.  Here: the restatements ARE the oracle's functions in float64 (values and autograd gradients to
1e-10 -- float64 rounding times at most 1e5 accumulations is 1e-11) and reproduce tests/golden/affine_bn.npz; the grid,
evaluated with the restated predicate and launch geometry, reaches both statistics kernels, the D > 256 chunk loops, a
short last workgroup and the grid-stride loop of every elementwise kernel; every bar is finite and nonzero; the kernels'
arithmetic modelled on the CPU (sums in double, bn_finalize_kernel, float32 normalisation) stays under every bar, and the
same model with the float partial sums the vector statistics kernel once kept does not, from mean / sd = 60 upwards."""
import numpy as np
import pytest
import torch

import bn_restatement as BR
from conftest import load_golden
from domain_helpers import float64

PIN = 1e-10


@pytest.fixture(scope="module")
def sweep(oracle):
    s = BR.Sweep(oracle)
    for section in BR.Sweep.SECTIONS:
        s.need(section)
    return s


# ---- the float64 restatements are the oracle's functions -------------------------------------------------------------------
def test_affine_restated(sweep, oracle):
    for c in sweep.affine:
        for inverse in (False, True):
            with float64():
                want = oracle.affine(c.z.double(), c.wide[:, :2 * c.D].double(), c.D, inverse)
            got = c.want[inverse]
            assert got[1].shape == (c.Mp, 1) and got[0].shape == (max(c.Mz, c.Mp), c.N, c.D)
            assert BR.err(got[0], want[0]) <= PIN and BR.err(got[1], want[1]) <= PIN


def test_affine_backward_restated(sweep, oracle):
    for c in sweep.affine_bwd:
        for inverse in (False, True):
            def loss(z_, p_):
                out, ld = oracle.affine(z_, p_, c.D, inverse)
                return (out * c.wz.double()).sum() + (ld * c.wl.double()).sum()

            with float64():
                gz, gp = BR.autograd(loss, (c.z, c.p), torch.float64)
            got = c.want[inverse]
            assert got[0].shape == c.z.shape and got[1].shape == c.p.shape
            assert BR.gerr(got[0], gz) <= PIN and BR.gerr(got[1], gp) <= PIN, (c.D, c.N, c.Mz, c.Mp, inverse)


def test_bn_apply_restated(sweep, oracle):
    for c in sweep.apply:
        for inverse in (False, True):
            z = c.z.double().requires_grad_()
            with float64():
                out, ld = (oracle.bn_inverse if inverse else oracle.bn_forward_frozen)(z, c.mean.double(), c.alpha.double())
            (out * c.wz.double()).sum().backward()
            got = c.want[inverse]
            assert BR.ferr(got[0], out) <= PIN and BR.err(got[1], ld) <= PIN and BR.ferr(got[2], z.grad) <= PIN


def test_bn_batch_restated(sweep, oracle):
    """On the batches with more than three rows: with two or three rows at mean / sd = 2000 the oracle's own float64
    quotient sqrt(var z) / sqrt(var z_norm) is no reference to 1e-10 (the sample spread can be 1e-6 of the mean)."""
    n = 0
    for c in sweep.batch + list(sweep.shards.values()):
        if c.rows <= BR.FEW_ROWS:
            continue
        assert tuple(c.want) == BR.EPSS  # eps = 0 runs on every batch with enough rows
        for eps in BR.EPSS:
            with float64(), torch.no_grad():
                want = oracle.bn_forward_batch(c.x[None].double(), eps=BR.ref_eps(eps))
                spelled = BR.bn_batch_expression(c.x[None].double(), eps)
            for key, e in list(BR.batch_errs(c.want[eps], want, c.D).items()) + list(BR.batch_errs(spelled, want, c.D).items()):
                assert e <= PIN, (c.D, c.rows, eps, key, e)
                n += 1
    assert n > 1000


def test_bn_batch_backward_restated(sweep, oracle):
    for c in sweep.batch_bwd + list(sweep.shard_bwd.values()):
        if c.rows <= BR.FEW_ROWS:
            continue
        with float64():
            gz, = BR.autograd(c.loss, (c.x,), torch.float64)
        for r, e in BR.grouped_gerr(c.want, gz, c.D).items():
            assert e <= 1e-9 if c.rows > 1e5 else e <= PIN, (c.D, c.rows, r, e)


def test_base_density_restated(oracle):
    g = torch.Generator().manual_seed(5)
    for D in BR.BASE_DS:
        x = torch.randn(3, 65, D, generator=g, dtype=torch.float64)
        want = torch.from_numpy(oracle.base_log_density_f64(x.numpy()))
        assert float(((BR.base64(x) - want).abs() / want.abs()).max()) <= PIN


def test_golden_through_the_restatement():
    """tests/golden/affine_bn.npz (the reference's float32 and float64 results) against the float64 restatements: the
    tolerances of tests/test_oracle_golden.py, as the measure of this sweep."""
    g = load_golden("affine_bn")
    for ci, (D, Mz, Mp, N, dt, extra) in enumerate(g["affine_meta"].tolist()):
        k = "a%02d_" % ci
        for inverse, name in ((False, "fwd"), (True, "inv")):
            out, ld = BR.affine64(g[k + "z"], g[k + "params"], D, inverse)
            tol = 1e-12 if g[k + "z"].dtype == np.float64 else 1e-5
            assert BR.err(out, g[k + "z_" + name]) <= tol and BR.err(ld, g[k + "ld_" + name]) <= tol
    for ci, (D, M, N) in enumerate(g["bn_meta"].tolist()):
        k = "b%02d_" % ci
        got = BR.bn_batch64(g[k + "z"], 1e-5)
        want = (g[k + "z_batch"], g[k + "ld_batch"], g[k + "mean"], g[k + "alpha"])
        for a, b in zip(got, want):
            assert BR.err(a, b) <= 1e-5
        for inverse, name in ((False, "frozen"), (True, "inv")):
            out, ld = BR.bn_apply64(g[k + "z2"], g[k + "mean"], g[k + "alpha"], inverse)
            assert BR.err(out, g[k + "z_" + name]) <= 1e-5 and BR.err(ld, g[k + "ld_" + name]) <= 1e-5


# ---- the grid reaches every path -----------------------------------------------------------------------------------------
def test_statistics_kernel_predicate():
    for D in BR.BATCH_DS:
        vec = D % 4 == 0 and D <= 1024
        assert BR.stats_route(D, 0x7F0000000000) == ("vec" if vec else "scalar")
        assert BR.stats_route(D, 0x7F0000000004) == "scalar"
    routes = {(BR.stats_route(D, off), D > 256) for D in BR.BATCH_DS for off in (0, 4)}
    assert routes == {("vec", False), ("vec", True), ("scalar", False), ("scalar", True)}  # D > 256: the chunk loop
    assert BR.stats_route(1024, 0) == "vec" and BR.stats_route(1028, 0) == "scalar"
    assert [BR.stats_route(D, 0) for D in BR.SHARD_DS] == ["scalar", "vec"]
    # lanes per row that do not divide 256 (idle lanes in every workgroup), and one lane per row
    assert {BR.stats_rpi(D, "vec") * (D // 4) for D in BR.BATCH_DS if BR.stats_route(D, 0) == "vec"} >= {255, 252, 195, 256}


def test_launch_geometry_restated():
    assert BR.stats_rpi(64, "vec") == 16 and BR.stats_rpi(1024, "vec") == 1 and BR.stats_rpi(12, "vec") == 85
    assert BR.stats_rpi(5, "scalar") == 51 and BR.stats_rpi(257, "scalar") == 1
    for D in BR.BATCH_DS:
        route = BR.stats_route(D, 0)
        rpi = BR.stats_rpi(D, route)
        assert BR.batch_rows(D) == (2, 3, 8 * rpi - 1, 8 * rpi, 8 * rpi + 1, 64 * rpi + 1)
        if route == "vec":  # one full iteration, one more row in a second workgroup, eight iterations and a tail
            assert [BR.stats_geometry(r, D, "vec")[0] for r in BR.batch_rows(D)] == [1, 1, 1, 1, 2, 9]
        assert any(M == 3 for r in BR.batch_rows(D) for M, N in BR.batch_layouts(r))  # three contexts
        assert any(M > 3 for r in BR.batch_rows(D) for M, N in BR.batch_layouts(r)) or D == 1024 or D == 1028
    D, rows = BR.BATCH_LONG
    blocks, rpb = BR.stats_geometry(rows, D, "vec")
    assert (blocks, rpb) == (512, 129) and rows % rpb != 0 and 8 * BR.stats_rpi(D, "vec") * 512 < rows  # cap and tail
    blocks, rpb = BR.stats_geometry(rows, D, "scalar")  # the same tensor at a 4-byte offset
    assert (blocks, rpb) == (257, 256) and rows % rpb != 0
    assert BR.stats_geometry(BR.BATCH_BWD_LONG[1], 5, "scalar") == (1024, 257) and BR.BATCH_BWD_LONG[1] % 257 != 0
    assert BR.affine_bwd_geometry(BR.AFFINE_BWD_LONG[1]) == (512, 257) and BR.AFFINE_BWD_LONG[1] % 257 != 0
    assert [BR.affine_bwd_geometry(N)[0] for N in BR.AFFINE_BWD_NS] == [1, 1, 1, 2]
    assert {D > 256 for D in BR.AFFINE_BWD_DS} == {D > 256 for D in BR.BATCH_BWD_DS} == {True, False}
    assert 257 in BR.AFFINE_BWD_DS and 257 in BR.BATCH_BWD_DS  # a one-feature second chunk
    assert {D > 64 for D in BR.AFFINE_DS} == {D > 64 for D in BR.APPLY_DS} == {True, False}  # the strided log-det loops


def test_grid_stride_loops_run(sweep):
    """At least one case of every elementwise kernel has more elements than 8192 workgroups of 256 threads."""
    big = BR.GRID_STRIDE
    assert max(max(c.Mz, c.Mp) * c.N * c.D for c in sweep.affine) > big                       # affine_kernel
    assert max(c.rows * c.D for c in sweep.apply) > big                                       # bn_apply(_backward)_kernel
    assert max(c.rows * c.D for c in sweep.batch) > big                                       # bn_normalize_kernel
    assert max(c.rows * c.D for c in sweep.batch_bwd) > big                                   # bn_batch_bwd_apply_kernel
    assert BR.BASE_LONG[1] * 4 > big and BR.base_blocks(BR.BASE_LONG[1]) == 8192              # base_log_density_kernel
    assert BR.elementwise_blocks(big + 1) == 8192 and BR.elementwise_blocks(big - 256) == 8191
    assert any(c.strided for c in sweep.affine)


# ---- the bars ------------------------------------------------------------------------------------------------------------
def test_bars_are_finite_and_nonzero(sweep):
    print("\n" + sweep.bars.table())
    groups = [BR.group(r, rows) for r in BR.RATIOS for rows in (2, 100)]
    want = {(q, d) for q in ("affine z", "affine ld", "affine g_z", "affine g_params", "apply z", "apply ld", "apply g_z")
            for d in ("fwd", "inv")}
    want |= {(q, g) for q in ("z_norm", "mean", "alpha", "batch g_z") for g in groups}
    want |= {("flow z", D) for D, *_ in BR.FLOWS} | {("flow log_q", D) for D, *_ in BR.FLOWS}
    assert want <= set(sweep.bars.noise)
    for key, v in sweep.bars.noise.items():
        assert np.isfinite(v) and v > 0.0, key
        if key[0] != "log_det" and not str(key[1]).endswith("-few"):  # float32 rounding, not a lower precision class
            assert 1e-9 < v < 1e-3, (key, v)


def _model_errs(c, eps, moments):
    return BR.batch_errs(BR.kernel_model(c.x, eps, moments), c.want[eps], c.D)


def test_double_sums_stay_under_the_bars(sweep):
    """The kernels' arithmetic on the CPU -- sums of x and x * x in double (the vector kernel's own order where an aligned
    tensor gets it), bn_finalize_kernel, the float32 normalisation -- meets every bar of the batch sweep: the bars ask for
    nothing a correct double formulation cannot give."""
    worst = 0.0
    for c in sweep.batch + list(sweep.shards.values()):
        vec = BR.stats_route(c.D, 0) == "vec" and c.rows * c.D <= 1 << 17
        for moments in ([BR.emulate_vec_moments(c.x, False)] if vec else []) + [BR.double_moments(c.x)]:
            for eps in c.want:
                for key, e in _model_errs(c, eps, moments).items():
                    assert e <= sweep.bars.bar(*key), (c.D, c.rows, eps, key, e, sweep.bars.bar(*key))
                    worst = max(worst, e / sweep.bars.bar(*key))
    print("largest error / bar of the double model: %.3f" % worst)
    few = [c for c in sweep.batch if c.rows <= BR.FEW_ROWS]
    assert 10 <= sum(0.0 in c.want for c in few) < len(few)  # eps = 0 at two and three rows too, where the draw allows


def test_float_partial_sums_fail_the_bars(sweep):
    """The planted fault: float32 partial sums over runs of 64 rows, as bn_stats_vec_kernel kept them before this sweep.
    At D = 8 and 1000 rows alpha misses its bar in every group from mean / sd = 60 upwards (and the model in double, on
    the same rows, does not): the bars catch the defect without a GPU."""
    c = sweep.shards[8]
    assert BR.stats_route(c.D, 0) == "vec" and set(BR.feature_groups(c.D)) == set(BR.RATIOS)
    for eps in BR.EPSS:
        bad = _model_errs(c, eps, BR.emulate_vec_moments(c.x, True))
        good = _model_errs(c, eps, BR.emulate_vec_moments(c.x, False))
        for r in BR.RATIOS:
            key = ("alpha", BR.group(r, c.rows))
            print("eps %g, mean / sd %d: alpha error %.1e with float partials, %.1e in double, bar %.1e"
                  % (eps, r, bad[key], good[key], sweep.bars.bar(*key)))
            assert good[key] <= sweep.bars.bar(*key)
            if r >= 60:
                assert bad[key] > sweep.bars.bar(*key)
    # and the raw moments: the float partials leave the summation bound of the sharded contract by decades
    want, terms = BR.moments64(c.x)
    bound = BR.sum_bound(c.rows, terms)
    assert (np.abs(BR.emulate_vec_moments(c.x, False)[:-1] - want[:-1]) <= bound).all()
    assert (np.abs(BR.emulate_vec_moments(c.x, True)[:-1] - want[:-1]) > 100.0 * bound).any()
