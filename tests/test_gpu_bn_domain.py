"""The Affine, BatchNorm and base-density kernels over their own domain against float64 -- generic_kernels.hip (affine_*,
bn_apply_*, bn_stats_kernel, bn_stats_vec_kernel, bn_finalize / normalize / count, base_log_density_kernel) and
backward_kernels.hip (affine_backward_*, bn_apply_backward_kernel, bn_batch_bwd_*) -- in the pattern of
tests/test_gpu_maf_domain.py.  Restatements, grid, inputs and bars: tests/bn_restatement.py; the host half, which pins the
restatements to the oracle and the grid's coverage without a GPU: tests/test_bn_host.py.

Reference: the float64 restatements on float64 copies of the inputs.  Bars: float32 results are held to 4 x the largest
error of the float32 reference (the oracle's expression on float32 tensors) in the same (quantity, group), measured on the
sweep's own inputs against the same float64 restatement; float64 results to rtol = atol = 1e-9
(tests/test_gpu_grad.py::test_affine_and_bn_grad).  Raw moments: rows x 2^-52 of sum |term|.  Base density: D x 2^-50
relative.  No bar comes from a kernel's output.

a  Affine forward / inverse, float32 and float64: D = 1, 2, 5, 63, 64, 65, 257 (the log-det loop strides from 65),
   (M_z, M_p, N) = (1,1,1), (3,3,7), (3,1,7), (1,4,7), (2,2,300); (1,1,33000) at D = 64 (the grid-stride loop); params as
   a column slice of a wider tensor (row stride 2 D + 7).
b  Affine backward, both directions, nonzero g_ld: D = 1, 5, 64, 255, 256, 257, 300 (a second feature chunk from 257),
   N = 1, 255, 256, 257 and 131,075 at D = 5 (512 workgroups of 257 rows); (M_z, M_p) = (3,3), (3,1) (three contexts
   accumulate into one row), (1,4).
c  Cached BatchNorm, both directions, forward and backward: D = 1, 5, 64, 257, rows 1, 7, 300 and 33,000 at D = 64;
   alpha from 1e-3 to 1e3, errors per feature.
d  Batch statistics: D = 1, 3, 4, 5, 8, 12, 60, 64, 68, 252, 256, 257, 260, 1024, 1028; rows 2, 3, 8 rpi - 1, 8 rpi,
   8 rpi + 1, 64 rpi + 1, and 65,541 at D = 64; every D % 4 == 0 tensor aligned (the vector kernel up to D = 1024) and as
   a view at a 4-byte offset (the scalar kernel); layouts (1, rows), (rows / k, k), (3, rows / 3); features cycle through
   (mean, sd) = (0,1), (1,1), (10,1), (3,.05), (10,.05), (100,1), (100,.05); eps = 1e-5, 1e-3 and, where no feature's
   sample mean / sd exceeds 2^13, 0.  Groups (quantity, mean / sd), two- and three-row batches in groups of their own.
   Constant features (0 and 1000.1, up to 32 rows): mean == c, z_norm == 0, alpha within a float32 ulp of sqrt(eps) --
   the reference divides 0 by 0 there and returns NaN; the closed form does not.  One row: refused, nothing cached.
e  The sharded halves (ops.HipBnShardKernels) at D = 6 (bn_count_kernel writes the count) and D = 8 (the vector kernel
   does): moments of the batch and of shards cut at 1, rows / 2, rows - 1 within the summation bound, an empty shard,
   normalize from summed moments, backward_sums and backward_apply with the global count.
f  Batch-statistics backward through BatchNorm.__call__, the loss on z_norm, log_det and the cached mean and alpha:
   D = 1, 5, 64, 257, 300, rows 2, 257, 262,151 at D = 5 and 33,000 at D = 64 (bn_batch_bwd_apply_kernel's stride loop).
g  Base density from float32 and float64: D = 1 .. 5, 63, 64, 65, 257, rows 1, 63, 64, 65 and 524,291 at D = 2.
h  NormFlow.forward(freeze_bn=False) at D = 64 and 32 (the folded chain: tnf_bn_batch_moments_f32 + bn_finalize) with
   the first Affine set to 3 + e^-3 x, so that the BatchNorm behind it sees mean / sd near 60; four base draws per shape
   (the float32 oracle's log_q error varies between 4e-8 and 1.4e-7 from draw to draw: one draw is no estimate of a
   group's noise).  log_q sits nearest its bar in the whole sweep: the chain keeps the per-context constant log-dets in
   a float32 running sum that passes through -3 D here, the oracle subtracts them from a float64 log_q one by one.

Before this sweep bn_stats_vec_kernel summed x and x^2 in float32 over runs of 64 rows.  Run against that build the sweep
recorded 1,912 missed comparisons, every one of them on the vector route: alpha in (d) from mean / sd = 10 upwards (1.8e-3
at 60, 1.2 at 2000 -- var_b clamped to 0, log_det infinite at eps = 0 -- largest at D = 1024 with 7 or 8 rows, where one
lane sums all rows), z_norm with it, the moments of (e) at D = 8 by 4e4 x the bound, g_z of (f) at D = 300 by up to
2,000 x its bar, log_q of (h) at D = 32; nothing on the scalar route missed.  DESIGN.md section 3.2a has the table.

Largest error / bar per sweep on the MI355X after the fix (the module prints them when it is done): a z 0.25, log_det
0.27; b g_z 0.29, g_params 0.87; c z 0.25, g_z 0.25, log_det 0.82; d alpha 0.09, mean 0.13, z_norm 0.25, log_det 0.56;
e moments 0.005 of the bound, alpha 0.06, z_norm 0.18, g_z 0.07; f g_z 0.24; g 0.25; h z 0.50, log_q 0.65."""
import numpy as np
import pytest
import torch

import bn_restatement as BR

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float64)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def sweep(oracle):
    """The cases and their bars: each section is built once, on the CPU, by the first test that needs it."""
    return BR.Sweep(oracle)


_WORST = {}  # (sweep, quantity) -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error / bar, %s %s: %.3f" % (*name, frac))


def under(sweep, letter, quantity, group, e, what):
    bar = sweep.bars.bar(quantity, group)
    _WORST[(letter, quantity)] = max(e / bar, _WORST.get((letter, quantity), 0.0))
    print("%s, %s [%s]: %.3e, %.3f of the bar" % (what, quantity, group, e, e / bar))
    assert np.isfinite(e) and e <= bar, "%s, %s [%s]: error %.3e exceeds %.3e" % (what, quantity, group, e, bar)


def close64(got, want):
    assert got.dtype == torch.float64
    torch.testing.assert_close(got.cpu(), want, **BR.F64_TOL)


# ---- a. Affine forward and inverse ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BR.AFFINE_DS)
def test_affine(tnf, sweep, D):
    sweep.need("affine")
    layer = tnf.Affine(D)
    for c in (c for c in sweep.affine if c.D == D):
        M = max(c.Mz, c.Mp)
        for dtype in DTYPES:
            wide = c.wide.to(dtype).cuda()
            p = wide[:, :2 * D] if c.strided else wide[:, :2 * D].contiguous()
            assert p.stride(0) == 2 * D + 7 if c.strided else p.is_contiguous()
            z = c.z.to(dtype).cuda()
            for inverse, d in ((False, "fwd"), (True, "inv")):
                what = "affine D%d (%d, %d, %d)%s %s" % (D, c.Mz, c.Mp, c.N, " strided" if c.strided else "", d)
                with torch.no_grad():
                    out, ld = (layer.inverse_and_log_det if inverse else layer.forward_and_log_det)(z, p)
                assert out.shape == (M, c.N, D) and ld.shape == (c.Mp, 1) and out.dtype == ld.dtype == dtype
                if dtype == torch.float64:
                    close64(out, c.want[inverse][0])
                    close64(ld, c.want[inverse][1])
                else:
                    under(sweep, "a", "affine z", d, BR.err(out, c.want[inverse][0]), what)
                    under(sweep, "a", "affine ld", d, BR.err(ld, c.want[inverse][1]), what)


# ---- b. Affine backward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BR.AFFINE_BWD_DS)
def test_affine_backward(tnf, sweep, D):
    sweep.need("affine_bwd")
    layer = tnf.Affine(D)
    for c in (c for c in sweep.affine_bwd if c.D == D):
        for dtype in DTYPES:
            for inverse, d in ((False, "fwd"), (True, "inv")):
                what = "affine backward D%d (%d, %d, %d) %s" % (D, c.Mz, c.Mp, c.N, d)
                z, p = c.z.to(dtype).cuda().requires_grad_(), c.p.to(dtype).cuda().requires_grad_()
                out, ld = (layer.inverse_and_log_det if inverse else layer.forward_and_log_det)(z, p)
                ((out * c.wz.to(dtype).cuda()).sum() + (ld * c.wl.to(dtype).cuda()).sum()).backward()
                assert z.grad.shape == z.shape and p.grad.shape == p.shape
                if dtype == torch.float64:
                    close64(z.grad, c.want[inverse][0])
                    close64(p.grad, c.want[inverse][1])
                else:
                    under(sweep, "b", "affine g_z", d, BR.gerr(z.grad, c.want[inverse][0]), what)
                    under(sweep, "b", "affine g_params", d, BR.gerr(p.grad, c.want[inverse][1]), what)


# ---- c. cached BatchNorm -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BR.APPLY_DS)
def test_bn_apply(tnf, sweep, D):
    sweep.need("apply")
    for c in (c for c in sweep.apply if c.D == D):
        bn = tnf.BatchNorm(D)
        bn.set_last_stats(c.mean.cuda(), c.alpha.cuda())
        assert D < 2 or float(c.alpha.max() / c.alpha.min()) == pytest.approx(1e6, rel=1e-5)
        for dtype in DTYPES:
            for inverse, d in ((False, "fwd"), (True, "inv")):
                what = "bn_apply D%d rows %d %s %s" % (D, c.rows, str(dtype)[6:], d)
                z = c.z.to(dtype).cuda().requires_grad_()
                out, ld = bn.inverse_and_log_det(z) if inverse else bn(z, use_last=True)
                (out * c.wz.to(dtype).cuda()).sum().backward()
                assert out.shape == z.shape and out.dtype == z.grad.dtype == dtype and ld.dim() == 0
                w_out, w_ld, w_gz = c.want[inverse]
                under(sweep, "c", "apply ld", d, BR.err(ld, w_ld), what)  # float32 whatever z is: the statistics are
                if dtype == torch.float64:
                    close64(out.detach(), w_out)
                    close64(z.grad, w_gz)
                else:
                    under(sweep, "c", "apply z", d, BR.ferr(out, w_out), what)
                    under(sweep, "c", "apply g_z", d, BR.ferr(z.grad, w_gz), what)


# ---- d. batch statistics -------------------------------------------------------------------------------------------------
def on_device(x, offset):
    """x (rows, D) on the device as a contiguous tensor whose first byte is `offset` floats past a 16-byte boundary"""
    flat = torch.empty(x.numel() + 4, dtype=torch.float32, device="cuda")
    v = flat[offset:offset + x.numel()]
    v.copy_(x.reshape(-1))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset
    return v


def check_batch(sweep, letter, c, eps, got, what):
    for (quantity, group), e in BR.batch_errs(got, c.want[eps], c.D).items():
        under(sweep, letter, quantity, group, e, what)


@pytest.mark.parametrize("D", BR.BATCH_DS)
def test_bn_batch(tnf, sweep, D):
    sweep.need("batch")
    for c in (c for c in sweep.batch if c.D == D):
        for offset in (0, 1) if D % 4 == 0 else (0,):
            v = on_device(c.x, offset)
            route = BR.stats_route(D, v.data_ptr())
            assert route == ("vec" if D % 4 == 0 and D <= 1024 and offset == 0 else "scalar")
            for eps in c.want:
                bn = tnf.BatchNorm(D, eps=eps)
                for M, N in BR.batch_layouts(c.rows) if eps == BR.EPSS[0] else [(1, c.rows)]:
                    what = "bn_batch D%d rows %d as (%d, %d) +%d B (%s) eps %g" % (D, c.rows, M, N, 4 * offset, route, eps)
                    z = v.view(M, N, D)
                    assert z.data_ptr() == v.data_ptr()
                    with torch.no_grad():
                        zn, ld = bn(z)
                    assert zn.shape == z.shape and ld.dim() == 0
                    check_batch(sweep, "d", c, eps, (zn, ld, bn.get_last_mean(), bn.get_last_alpha()), what)


@pytest.mark.parametrize("value", [0.0, 1000.1])
def test_bn_batch_constant_features(tnf, value):
    """n c and n c^2 are exact in double for a float32 c and n <= 32, so every correct double formulation gives mean == c,
    var_b == 0, z_norm == 0 and alpha = sqrt(eps) to the rounding of its float32 output.  The reference returns NaN here
    (bijectors.py:401-417 divides by the variance of z_norm, which is 0): a divergence on purpose."""
    c32 = np.float32(value)
    for D in (8, 5, 64):
        for rows in (2, 7, 32):
            for offset in (0, 1) if D % 4 == 0 else (0,):
                v = on_device(torch.full((rows, D), float(c32)), offset)
                for eps in BR.EPSS[:2]:
                    bn = tnf.BatchNorm(D, eps=eps)
                    with torch.no_grad():
                        zn, ld = bn(v.view(1, rows, D))
                    mean, alpha = bn.get_last_mean().cpu().numpy(), bn.get_last_alpha().cpu().numpy()
                    want = np.float32(np.sqrt(np.float64(np.float32(eps))))
                    assert (mean == c32).all() and float(zn.abs().max()) == 0.0, (D, rows, offset, eps)
                    assert (np.abs(alpha - want) <= np.spacing(want)).all(), (D, rows, offset, eps, alpha, want)
                    assert float(ld) == pytest.approx(-D * np.log(np.float64(want)), rel=1e-5)


def test_bn_batch_refuses_one_row(tnf):
    bn = tnf.BatchNorm(8)
    mean, alpha, version = bn.get_last_mean(), bn.get_last_alpha(), bn._version
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(torch.ones(1, 1, 8).cuda())
    assert bn.get_last_mean() is mean and bn.get_last_alpha() is alpha and bn._version == version
    assert torch.equal(mean, torch.zeros(8)) and torch.equal(alpha, torch.ones(8))


# ---- e. the sharded halves -----------------------------------------------------------------------------------------------
def check_moments(got, x, what):
    """[sum x | sum x^2 | count] of x (rows, D) within rows x 2^-52 of sum |term|; -> got as numpy"""
    D = x.shape[-1]
    got = got.cpu().numpy()
    want, terms = BR.moments64(x)
    bound = BR.sum_bound(x.shape[0], terms)
    excess = np.abs(got[:2 * D] - want[:2 * D]) - bound
    worst = float((np.abs(got[:2 * D] - want[:2 * D]) / np.maximum(bound, 1e-300)).max()) if x.shape[0] else 0.0
    _WORST[("e", "moments")] = max(worst, _WORST.get(("e", "moments"), 0.0))
    print("%s: %.3f of the summation bound" % (what, worst))
    assert got.shape == (2 * D + 1,) and (excess <= 0.0).all(), "%s: %.3f of the summation bound" % (what, worst)
    assert got[2 * D] == x.shape[0], "%s: count %r" % (what, got[2 * D])
    return got


@pytest.mark.parametrize("D", BR.SHARD_DS)
def test_bn_shard_halves(tnf, sweep, D):
    sweep.need("batch")
    sweep.need("batch_bwd")
    K = tnf.ops.HipBnShardKernels
    c, rows = sweep.shards[D], BR.SHARD_ROWS
    z = c.x.cuda()[None]
    assert BR.stats_route(D, z.data_ptr()) == ("vec" if D == 8 else "scalar")
    whole = check_moments(K.moments(z), c.x, "moments D%d, the batch" % D)
    assert not K.moments(z[:, :0]).cpu().numpy().any()  # an empty shard: zeros, count 0
    for cut in (1, rows // 2, rows - 1):
        parts = [z[:, :cut], z[:, cut:]]
        assert all(p.is_contiguous() for p in parts)
        moms = [K.moments(p) for p in parts]
        for p, m in zip(parts, moms):
            check_moments(m, p[0].cpu(), "moments D%d, a shard of %d rows" % (D, p.shape[1]))
        total = moms[0] + moms[1]
        assert float(total[2 * D]) == rows
        want, terms = BR.moments64(c.x)
        assert (np.abs(total.cpu().numpy() - want)[:2 * D] <= BR.sum_bound(rows, terms)).all()
        assert (np.abs(total.cpu().numpy() - whole)[:2 * D] <= 2 * BR.sum_bound(rows, terms)).all()
        for eps in BR.EPSS[:2]:
            outs = [K.normalize(p, total, eps) for p in parts]
            for o in outs:  # every shard ends up with the statistics of the whole batch
                assert torch.equal(o[2], outs[0][2]) and torch.equal(o[3], outs[0][3]) and torch.equal(o[1], outs[0][1])
            zn = torch.cat([o[0] for o in outs], 1)
            check_batch(sweep, "e", c, eps, (zn, *outs[0][1:]), "shards D%d cut at %d eps %g" % (D, cut, eps))
    # backward: local sums, summed, applied with the global count
    b = sweep.shard_bwd[D]
    x, g = b.x.cuda(), b.w.z.cuda()
    zn, _, _, alpha = K.normalize(x, K.moments(x), b.eps)
    cut = rows // 2
    zs, gs = [zn[:, :cut].contiguous(), zn[:, cut:].contiguous()], [g[:, :cut].contiguous(), g[:, cut:].contiguous()]
    sums = [K.backward_sums(a, b_) for a, b_ in zip(zs, gs)]
    for s, a, b_ in zip(sums, zs, gs):
        a64, g64 = a[0].double().cpu().numpy(), b_[0].double().cpu().numpy()  # float32 x float32 is exact in double
        want = np.concatenate([g64.sum(0), (g64 * a64).sum(0)])
        bound = BR.sum_bound(a64.shape[0], np.concatenate([np.abs(g64).sum(0), np.abs(g64 * a64).sum(0)]))
        assert (np.abs(s.cpu().numpy() - want) <= bound).all()
    total = sums[0] + sums[1]
    total[D:] += b.w.ld  # the log-det's gradient rides with sum g x^ (ops._BnBatchShardedFn)
    count = torch.tensor([float(rows)], dtype=torch.float64, device="cuda")
    gz = torch.cat([K.backward_apply(a, b_, None, alpha, total, count) for a, b_ in zip(zs, gs)], 1)
    gz = gz + (b.w.mean.cuda() / rows + zn * (b.w.alpha.cuda() / rows))  # the cached statistics' gradients, as ops.py adds them
    for group, e in BR.grouped_gerr(gz, b.want, D).items():
        under(sweep, "e", "batch g_z", group, e, "sharded backward D%d" % D)


# ---- f. batch-statistics backward ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BR.BATCH_BWD_DS)
def test_bn_batch_backward(tnf, sweep, D):
    sweep.need("batch_bwd")
    for c in (c for c in sweep.batch_bwd if c.D == D):
        bn = tnf.BatchNorm(D, eps=c.eps)
        z = c.x.cuda().requires_grad_()
        zn, ld = bn(z)
        mean, alpha = bn.get_last_mean(), bn.get_last_alpha()
        assert mean.requires_grad and alpha.requires_grad  # cached WITH their graph (bijectors.py:414-415)
        w = c.w
        ((zn * w.z.cuda()).sum() + w.ld * ld + (mean * w.mean.cuda()).sum() + (alpha * w.alpha.cuda()).sum()).backward()
        for group, e in BR.grouped_gerr(z.grad, c.want, D).items():
            under(sweep, "f", "batch g_z", group, e, "bn_batch backward D%d rows %d" % (D, c.rows))


# ---- g. base density -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BR.BASE_DS)
def test_base_density(tnf, D):
    g = torch.Generator().manual_seed(D)
    for rows in BR.BASE_ROWS + ((BR.BASE_LONG[1],) if D == BR.BASE_LONG[0] else ()):
        x = torch.randn(1, rows, D, generator=g, dtype=torch.float64)
        for dtype in DTYPES:
            xin = x.to(dtype)
            got = tnf.ops.base_log_density_f64(xin.cuda())
            want = BR.base64(xin)
            assert got.dtype == torch.float64 and got.shape == (1, rows)
            e = float(((got.cpu() - want).abs() / want.abs()).max())
            _WORST[("g", "base density")] = max(e / (D * 2.0 ** -50), _WORST.get(("g", "base density"), 0.0))
            assert e <= D * 2.0 ** -50, "base density D%d rows %d %s: %.3e" % (D, rows, dtype, e)


# ---- h. carry-through ----------------------------------------------------------------------------------------------------
def test_flow_forward_with_a_concentrated_batch(tnf, sweep):
    sweep.need("flow")
    for c in sweep.flows:
        nf = tnf.NormFlow(c.D, False, "coupling", c.S, c.L, c.U)
        nf.params = c.params.cuda()
        ratios = [float((m.abs() / a).max()) for m, a in c.stats]
        assert max(ratios) > 50.0, ratios  # a BatchNorm of the stack sees mean / sd near 60
        z32 = torch.as_tensor(c.omega).float().cuda()
        assert nf._route("forward", z32, nf.params, False).family == "batch_chain"
        with torch.no_grad():
            z, lq = nf._forward_from(c.omega, nf.params, freeze_bn=False)
        assert lq.dtype == torch.float64
        what = "NormFlow.forward D%d S%d N%d" % (c.D, c.S, c.N)
        under(sweep, "h", "flow z", c.D, BR.err(z, c.z), what)
        under(sweep, "h", "flow log_q", c.D, BR.err(lq, c.lq), what)
        for i, (b, (m, a)) in enumerate(zip(nf._bn_layers(), c.stats)):
            e = float(((b.get_last_alpha().cpu().double() - a).abs() / a).max())
            print("%s: BatchNorm %d, mean / sd up to %.0f: alpha off by %.1e" % (what, i, ratios[i], e))
