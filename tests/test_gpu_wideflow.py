"""The whole-flow wide kernel (include/tnf_wideflow.h, csrc/flow_wide.hip) through the C ABI and through NormFlow with
`wide_flow = True`, against the CPU oracle run in float64 on float64 copies of the same float32 inputs.

Error measure: `err` of tests/maf_restatement.py, max |got - want| / max(1, max |want| over the case).  Bars: per group
(quantity, L), 4 x the largest error of the float32 restatement (tests/wideflow_restatement.py) against the float64 oracle
on the sweep's own inputs -- the rule of tests/test_gpu_wide_domain.py: room for another summation order and 1-ulp
exp2 / rcp, not for a lower precision class.  They are computed on the CPU when the sweep is built and printed with each
case's error / bar; no bar comes from a kernel's output.  Inputs, grid and references: tests/wideflow_restatement.py.

Worst error / bar per group over the sweep (C ABI and NormFlow), the tile walk and the layout tests, MI355X:
             lp     z0     sld    zf     sldf
    L = 1    0.36   0.28   0.22   0.34   0.28
    L = 2    0.26   0.54   0.58   0.23   0.33
    L = 3    0.17   0.17   0.15   0.16   0.13
    L = 5    0.90   0.75   0.21   0.19   0.30
The round trip: 0.19 and 0.20 of its bars; the conditional estimator: at most 0.01.

The L = 5 group has one case, D8-S1-L5-U20, so its bars are 4 x one sample of the restatement's noise (lp 9.22e-07,
z0 1.48e-06).  With the plain hardware activation in every layer the kernel missed it in the row layout (3, 1, 33):
lp 4.13e-06 against 3.69e-06.  From L = 4 on the kernel therefore refines the activation's reciprocal by one Newton step
(csrc/wide_flow_tile.h sig2_nr): lp 3.33e-06, z0 4.41e-06 against 5.90e-06."""
import pytest
import torch

import domain_helpers as H
import wideflow_restatement as W
from domain_helpers import float64
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
ALL = dict(want_lp=True, want_z0=True, want_sld=True)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def wf(tnf):
    from torch_nf_amd import wideflow_ops

    return wideflow_ops


def wide_counts():
    torch.cuda.synchronize()
    return [lib.tnf_wide_flow_launch_count(0), lib.tnf_wide_flow_launch_count(1)]


def other_counts():
    """The counter spaces of the other families that have one."""
    return [lib.tnf_ctx_flow_launch_count(0), lib.tnf_ctx_flow_launch_count(1), lib.tnf_ctx_sample_launch_count()]


class one_launch(object):
    """`with one_launch(lp, fwd)`: the block moves the two new counters by exactly (lp, fwd), no diag family and no other
    family's own counter."""

    def __init__(self, lp, fwd):
        self.want = [lp, fwd]

    def __enter__(self):
        self.wide, self.diag, self.other = wide_counts(), H.counts(), other_counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(wide_counts(), self.wide)] == self.want
            assert H.launched(self.diag) == {} and other_counts() == self.other
        return False


class Sweep:
    """Every case with its references, built once, and `noise`: {(quantity, L): the float32 restatement's largest error
    against the float64 oracle over the group's cases}."""

    def __init__(self, oracle):
        self.oracle, self.noise, self.worst = oracle, {}, {}
        self.cases = {s: W.Case(oracle, *s) for s in W.sweep_shapes()}
        self.walk = {HT: W.Case(oracle, *s, rows=(1, W.WALK_N), layouts=[(1, 1)]) for HT, s in W.WALK_SHAPES.items()}
        for c in list(self.cases.values()) + list(self.walk.values()):
            for k, v in c.noise().items():
                key = (k, c.shape[2])
                self.noise[key] = max(v, self.noise.get(key, 0.0))
        print("noise of the float32 restatement against float64:\n" + "\n".join(
            "%-5s L=%d  noise %.2e  bar %.2e" % (k, L, v, 4 * v) for (k, L), v in sorted(self.noise.items())))

    def bar(self, k, L):
        return 4.0 * self.noise[(k, L)]

    def check(self, c, got, want, what):
        """Every quantity of `got` within its group's bar; prints error / bar."""
        sc, L, bad = c.scale(), c.shape[2], []
        for k, v in got.items():
            assert v.shape == want[k].shape and bool(torch.isfinite(v).all()), (what, k)
            e, bar = W.err(v, want[k], sc[k]), self.bar(k, L)
            self.worst[(k, L)] = max(self.worst.get((k, L), 0.0), e / bar)
            print("%s %-4s err %.2e / bar %.2e = %.2f" % (what, k, e, bar, e / bar))
            if not e <= bar:
                bad.append((what, k, e, bar))
        assert not bad, bad


@pytest.fixture(scope="module")
def sw(oracle):
    s = Sweep(oracle)
    yield s
    print("worst error / bar per group:\n" + "\n".join("%-5s L=%d  %.2f" % (k, L, v) for (k, L), v in sorted(s.worst.items())))


def dev(c, Mz, Mp, N=None):
    z, p = c.inputs(Mz, Mp, N)
    return z.contiguous().cuda(), p.contiguous().cuda(), c.stat[0].cuda(), c.stat[1].cuda()


def inverse(wf, c, Mz, Mp, N=None, **kw):
    lp, z0, sld = wf.wide_flow_log_prob_raw(*dev(c, Mz, Mp, N), *c.shape, **(kw or ALL))
    return {k: v for k, v in (("lp", lp), ("z0", z0), ("sld", sld)) if v is not None}


def forward(wf, c, Mz, Mp, N=None):
    zf, sldf = wf.wide_flow_forward_raw(*dev(c, Mz, Mp, N), *c.shape)
    return dict(zf=zf, sldf=sldf)


def make_nf(tnf, c):
    D, S, L, U = c.shape
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    assert (nf.num_layers, nf.num_units, nf.D_params) == (L, U, W.flow_params(*c.shape))
    for i, b in enumerate(nf._bn_layers()):
        b.set_last_stats(c.stat[0][i], c.stat[1][i])
    nf.wide_flow = True
    return nf


# ---- the sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.sweep_shapes(), ids=W.case_id)
def test_sweep_through_the_abi(wf, sw, shape):
    """Every row layout, both directions, every output: one launch each."""
    c = sw.cases[shape]
    for Mz, Mp, N in W.ROWS + W.LP_ONLY_ROWS:
        what = "%s (%d, %d, %d)" % (W.case_id(shape), Mz, Mp, N)
        with one_launch(1, 0):
            got = inverse(wf, c, Mz, Mp, N)
        sw.check(c, got, c.want(Mz, Mp, N), what)
        if (Mz, Mp, N) in W.ROWS:
            with one_launch(0, 1):
                got = forward(wf, c, Mz, Mp, N)
            sw.check(c, got, c.want(Mz, Mp, N), what)


@pytest.mark.parametrize("shape", W.sweep_shapes(), ids=W.case_id)
def test_sweep_through_normflow(tnf, sw, shape):
    """log_prob, inverse_and_log_det and frozen sampling of NormFlow with the switch on: one launch of the new kernel each;
    with the switch off the same call moves today's counters instead."""
    c = sw.cases[shape]
    nf = make_nf(tnf, c)
    for Mz, Mp in ((3, 3), (3, 1)):
        what = "NormFlow %s (%d, %d)" % (W.case_id(shape), Mz, Mp)
        z, p, _, _ = dev(c, Mz, Mp)
        want = c.want(Mz, Mp, W.N_FULL)
        with torch.no_grad():
            with one_launch(1, 0):
                lp = nf.log_prob(z, p)
            with one_launch(1, 0):
                z0, sld = nf.inverse_and_log_det(z, p)
            got = dict(lp=lp, z0=z0, sld=sld)
            if Mp > 1 and shape[0] in (8, 16, 24):  # sampling, several rows: left to the wide chain
                wide = wide_counts()
                nf._forward_from(z, p, freeze_bn=True)
                assert wide_counts() == wide
            else:
                with one_launch(0, 1):
                    zf, lq = nf._forward_from(z, p, freeze_bn=True)
                assert lq.dtype == torch.float64
                base = torch.tensor(sw.oracle.base_log_density_f64(c.inputs(Mz, Mp)[0].double().numpy()))
                got.update(zf=zf, sldf=base - lq.cpu())
            sw.check(c, got, want, what)
    with torch.no_grad():
        nf.wide_flow = False
        wide, diag = wide_counts(), H.counts()
        nf.log_prob(z, p)
        assert wide_counts() == wide
        if shape[0] % 8 == 0:  # today's wide per-layer chain counts its launches; the per-bijector composition has no counter
            assert H.launched(diag).get(L_.DIAG_COUPLING_WIDE, 0) > 0


@pytest.mark.parametrize("M", [1, W.WALK_M])
@pytest.mark.parametrize("HT", [1, 2])
def test_tile_walk(wf, sw, HT, M):
    """N = 2,065: 130 tiles, the last with one row.  M = 1: 17 workgroups of 8 waves, six waves without a tile.  M = 512: the
    x-grid is clamped to one workgroup per row, whose waves walk 16 or 17 tiles.  Block m holds the rows of block 0 rotated
    by m, so every row of the batch has its reference in the one float64 run."""
    c = sw.walk[HT]
    N = W.WALK_N
    assert W.grid_x(N, M) == (17 if M == 1 else 1)
    z, p, mean, alpha = dev(c, 1, 1)
    idx = (torch.arange(N)[None, :] + torch.arange(M)[:, None]) % N
    zb, pb = z[0][idx.cuda()].contiguous(), p.expand(M, -1).contiguous()
    want = {k: v[0][idx] for k, v in c.want(1, 1, N).items()}
    what = "walk %s M=%d" % (W.case_id(c.shape), M)
    with one_launch(1, 0):
        lp, z0, sld = wf.wide_flow_log_prob_raw(zb, pb, mean, alpha, *c.shape, **ALL)
    sw.check(c, dict(lp=lp, z0=z0, sld=sld), want, what)
    with one_launch(0, 1):
        zf, sldf = wf.wide_flow_forward_raw(zb, pb, mean, alpha, *c.shape)
    sw.check(c, dict(zf=zf, sldf=sldf), want, what)


def test_subsets_of_the_outputs(wf, sw):
    """Every output subset of both entries is the same bits as the full call."""
    for shape in ((5, 2, 3, 17), (63, 2, 2, 32)):
        c = sw.cases[shape]
        full = inverse(wf, c, 3, 3)
        for kw, keys in ((dict(want_lp=True), ("lp",)), (dict(want_lp=False, want_z0=True, want_sld=True), ("z0", "sld")),
                         (dict(want_lp=False, want_sld=True), ("sld",)), (dict(want_lp=False, want_z0=True), ("z0",))):
            with one_launch(1, 0):
                got = inverse(wf, c, 3, 3, **kw)
            assert tuple(got) == keys and all(torch.equal(got[k], full[k]) for k in keys)
        z, p, mean, alpha = dev(c, 3, 3)
        zf, sldf = wf.wide_flow_forward_raw(z, p, mean, alpha, *shape)
        for want_z, want_s in ((True, False), (False, True)):
            zo = torch.empty_like(zf) if want_z else None
            so = torch.empty_like(sldf) if want_s else None
            with one_launch(0, 1):
                L_.check(lib.tnf_wide_flow_forward_f32(z.data_ptr(), p.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                                       zo.data_ptr() if want_z else None, so.data_ptr() if want_s else None,
                                                       3, 3, W.N_FULL, *shape, p.stride(0), L_.stream_ptr()))
            assert torch.equal(zo, zf) if want_z else torch.equal(so, sldf)


@pytest.mark.parametrize("HT", [1, 2])
def test_log_prob_of_the_samples(wf, sw, HT):
    """log_prob(forward(omega)) against log N(omega) - sum_log_det of the float64 oracle.  Bar: 4 x the error of the same
    composition in the float32 restatement (its log_prob on its own forward's z) against the same float64 value."""
    shape = {1: (5, 2, 3, 17), 2: (63, 2, 2, 32)}[HT]
    c = sw.cases[shape]
    z, p, mean, alpha = dev(c, 3, 3)
    omega, params = c.inputs(3, 3)
    want = torch.tensor(sw.oracle.base_log_density_f64(omega.double().numpy())) - c.want(3, 3, W.N_FULL)["sldf"]
    with torch.no_grad():
        z32 = W.wide_flow_forward(omega, params, *shape, c.stat)[0]
        noise = W.err(W.wide_flow_log_prob(z32, params, *shape, c.stat)[0], want)
    zf, _ = wf.wide_flow_forward_raw(z, p, mean, alpha, *shape)
    lp = wf.wide_flow_log_prob_raw(zf, p, mean, alpha, *shape)[0]
    e = W.err(lp, want)
    print("round trip %s: err %.2e / bar %.2e" % (W.case_id(shape), e, 4 * noise))
    assert e <= 4 * noise


# ---- memory discipline -------------------------------------------------------------------------------------------------------
GUARD = -777.25


@pytest.mark.parametrize("shape", [(5, 2, 3, 17), (8, 5, 1, 33)], ids=W.case_id)
def test_rows_offsets_and_guards(wf, sw, shape):
    """A parameter row stride 7 floats longer than the row with NaNs behind each row; z at a 4-byte offset inside a
    NaN-filled buffer (D = 8: the float4 path must not be taken); every output inside a larger buffer whose guard regions
    are bit-unchanged afterwards."""
    c = sw.cases[shape]
    D, M, N, P = shape[0], 3, W.N_FULL, W.flow_params(*shape)
    z, p = c.inputs(M, M)
    pbuf = torch.full((M, P + 7), float("nan"))
    pbuf[:, :P] = p
    zbuf = torch.full((M * N * D + 8,), float("nan"))
    zbuf[1:1 + M * N * D] = z.reshape(-1)
    pbuf, zbuf, mean, alpha = pbuf.cuda(), zbuf.cuda(), c.stat[0].cuda(), c.stat[1].cuda()
    zin = zbuf[1:]
    assert zin.data_ptr() % 16 == 4 and pbuf.stride(0) == P + 7

    def guarded(n, lead):
        buf = torch.full((n + lead + 9,), GUARD, device="cuda")
        return buf, buf[lead:lead + n]

    for fwd in (False, True):
        bufs = dict(lp=guarded(M * N, 4), z=guarded(M * N * D, 3), sld=guarded(M * N, 1))
        with one_launch(int(not fwd), int(fwd)):
            if fwd:
                L_.check(lib.tnf_wide_flow_forward_f32(zin.data_ptr(), pbuf.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                                       bufs["z"][1].data_ptr(), bufs["sld"][1].data_ptr(), M, M, N, *shape,
                                                       P + 7, L_.stream_ptr()))
            else:
                L_.check(lib.tnf_wide_flow_log_prob_f32(zin.data_ptr(), pbuf.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                                        bufs["lp"][1].data_ptr(), bufs["z"][1].data_ptr(),
                                                        bufs["sld"][1].data_ptr(), M, M, N, *shape, P + 7, L_.stream_ptr()))
        torch.cuda.synchronize()
        names = dict(z="zf", sld="sldf") if fwd else dict(lp="lp", z="z0", sld="sld")
        got = {}
        for k, name in names.items():
            buf, view = bufs[k]
            inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
            inside[view.storage_offset():view.storage_offset() + view.numel()] = True
            assert bool((buf[~inside] == GUARD).all()), "%s: a guard float changed" % name
            got[name] = view.reshape((M, N, D) if k == "z" else (M, N)).clone()
        sw.check(c, got, c.want(M, M, N), "offset %s %s" % (W.case_id(shape), "forward" if fwd else "inverse"))
        # the same bits as the aligned, densely packed call
        ref = forward(wf, c, M, M) if fwd else inverse(wf, c, M, M)
        assert all(torch.equal(got[k], ref[k]) for k in got)


def test_two_runs_are_bit_identical(wf, sw):
    for shape in ((33, 1, 1, 20), (3, 1, 2, 64)):
        c = sw.cases[shape]
        a, b = inverse(wf, c, 3, 3), inverse(wf, c, 3, 3)
        assert all(torch.equal(a[k], b[k]) for k in a)
        a, b = forward(wf, c, 3, 1), forward(wf, c, 3, 1)
        assert all(torch.equal(a[k], b[k]) for k in a)
    c = sw.walk[1]
    z, p, mean, alpha = dev(c, 1, 1)
    a = wf.wide_flow_log_prob_raw(z, p, mean, alpha, *c.shape, **ALL)
    b = wf.wide_flow_log_prob_raw(z, p, mean, alpha, *c.shape, **ALL)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_capture(wf, sw):
    """One log_prob call captured on a single stream (no parallel branches) replays to the same bits."""
    c = sw.cases[(63, 2, 2, 32)]
    args = dev(c, 3, 3) + c.shape
    eager = wf.wide_flow_log_prob_raw(*args)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        wf.wide_flow_log_prob_raw(*args)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lp = wf.wide_flow_log_prob_raw(*args)[0]
    before = wide_counts()
    lp.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert wide_counts() == before  # a replay runs the captured kernel; no call reaches the host launcher
    assert torch.equal(lp, eager)


def test_conditional_estimator_calls(tnf, sw, oracle):
    """NormFlow(4, True, 'coupling', 1, 2, 20) inside a ConditionalDensityEstimator, the switch on: cde.log_prob(z (M, 33, 4),
    x) and cde.sample(x, 33) are one launch of the new kernel each.  Reference: the float64 oracle on float64 copies of the
    parameter rows the conditioner hands the flow (the rows the switch-off call uses).  Bars: the L = 2 groups, or 4 x the
    float32 restatement's error on these very inputs where that is larger (the rows follow the conditioner's law, not the
    sweep's)."""
    shape, M, N = W.CDE_SHAPE, 5, 33
    D = shape[0]
    nf, cde = H._cde(tnf, D, shape[1], shape[2], 100, seed=4, U=shape[3])
    assert (nf.num_units, nf.wide_flow) == (20, False)
    g = torch.Generator().manual_seed(4)
    x, z = torch.randn(M, 8, generator=g), torch.randn(M, N, D, generator=g)
    gen = torch.Generator(device="cuda").manual_seed(11)
    omega = torch.randn((M, N, D), device="cuda", dtype=torch.float32, generator=gen).cpu()
    with torch.no_grad():
        params = cde._params_for(x.cuda()).cpu()
        stat = (torch.stack([b.get_last_mean().cpu() for b in nf._bn_layers()]),
                torch.stack([b.get_last_alpha().cpu() for b in nf._bn_layers()]))
        with float64():
            st = W.stats_list(stat, torch.float64)
            lp_w = oracle.flow_log_prob(z.double(), params.double(), *shape, st)
            zf_w, lq_w, _ = oracle.flow_forward(omega.double().numpy(), params.double(), *shape, st)
        fold = dict(lp=W.wide_flow_log_prob(z, params, *shape, stat)[0])
        fold["zf"], sldf32, _ = W.wide_flow_forward(omega, params, *shape, stat)
        fold["lq"] = torch.tensor(oracle.base_log_density_f64(omega.double().numpy())) - sldf32.double()
        want = dict(lp=lp_w, zf=zf_w, lq=lq_w)
        bars = {k: 4 * max(W.err(fold[k], want[k]), sw.noise[(dict(lq="sldf").get(k, k), 2)]) for k in want}

        wide, diag = wide_counts(), H.counts()
        cde.log_prob(z.cuda(), x.cuda())
        assert wide_counts() == wide and H.launched(diag) == {}  # switch off: the composition, which has no counter
        nf.wide_flow = True
        with one_launch(1, 0):
            lp = cde.log_prob(z.cuda(), x.cuda())
        gen.manual_seed(11)
        with one_launch(0, 1):
            zs, lq = cde.sample(x.cuda(), N, generator=gen)
    got = dict(lp=lp, zf=zs, lq=lq)
    for k in want:
        e = W.err(got[k], want[k])
        print("cde %-2s err %.2e / bar %.2e" % (k, e, bars[k]))
        assert got[k].shape == want[k].shape and e <= bars[k], k
