"""The streamed whole-flow wide kernel (include/tnf_widestream.h, csrc/flow_wide_stream.hip) through the C ABI and through
NormFlow with `wide_flow_streamed = True`, against the CPU oracle run in float64 on float64 copies of the same float32
inputs, and bit for bit against the resident kernel (csrc/flow_wide.hip) where both apply.

Error measure and bars: the rule of tests/test_gpu_wideflow.py.  `err` of tests/maf_restatement.py,
max |got - want| / max(1, max |want| over the case); per group (quantity, L) the bar is 4 x the largest error of the float32
restatement (tests/wideflow_restatement.py) against the float64 oracle on the sweep's own inputs -- the sixteen cases of
widestream_restatement.SWEEP, none of which the resident kernel accepts, and the two group-walk cases.  The bars are
computed on the CPU when the sweep is built and printed with each case's error / bar; no bar comes from a kernel's
output.  Every L has at least two cases.

Worst error / bar per group over the sweep, the group walk and the layout tests, MI355X:
             lp     z0     sld    zf     sldf
    L = 1    0.37   0.39   0.20   0.28   0.46
    L = 2    0.25   0.23   0.30   0.18   0.21
    L = 3    0.19   0.36   0.15   0.12   0.27
    L = 4    0.08   0.18   0.30   0.37   0.10
    L = 5    0.13   0.21   0.28   0.22   0.21
The round trip: 0.56 and 0.25 of its bars; the headline model and the conditional estimator: at most 0.10 of theirs
against float64; switch on against switch off: at most 0.76 of two bars (log_q behind a ToInterval layer)."""
import pytest
import torch

import domain_helpers as H
import wideflow_restatement as W
import widestream_restatement as R
from domain_helpers import float64
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
ALL = dict(want_lp=True, want_z0=True, want_sld=True)
GUARD = -777.25


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def ws(tnf):
    from torch_nf_amd import widestream_ops

    yield widestream_ops
    widestream_ops.set_tiles(0)


@pytest.fixture(scope="module")
def wf(tnf):
    from torch_nf_amd import wideflow_ops

    return wideflow_ops


class forced_tiles(object):
    """`with forced_tiles(ws, T)`: T tiles per wave for the block, the rule afterwards."""

    def __init__(self, ws, T):
        self.ws, self.T = ws, T

    def __enter__(self):
        self.ws.set_tiles(self.T)

    def __exit__(self, *exc):
        self.ws.set_tiles(0)
        return False


def stream_counts():
    torch.cuda.synchronize()
    return [lib.tnf_wide_flow_stream_launch_count(0), lib.tnf_wide_flow_stream_launch_count(1)]


def other_counts():
    """The counter spaces of the other families that have one."""
    return [lib.tnf_wide_flow_launch_count(0), lib.tnf_wide_flow_launch_count(1), lib.tnf_ctx_flow_launch_count(0),
            lib.tnf_ctx_flow_launch_count(1), lib.tnf_ctx_sample_launch_count(), lib.tnf_ctx_wide_launch_count(0),
            lib.tnf_ctx_wide_launch_count(1)]


class one_launch(object):
    """`with one_launch(lp, fwd)`: the block moves the two new counters by exactly (lp, fwd), no diag family and no other
    family's own counter."""

    def __init__(self, lp, fwd):
        self.want = [lp, fwd]

    def __enter__(self):
        self.mine, self.diag, self.other = stream_counts(), H.counts(), other_counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(stream_counts(), self.mine)] == self.want
            assert H.launched(self.diag) == {} and other_counts() == self.other
        return False


WALK_N = R.walk_N(max(R.SHIPPED_TILES))
WALK_LAYOUTS = [(R.WALK_M, R.WALK_M), (R.WALK_M, 1), (1, 1)]


class Sweep:
    """Every case with its references, built once, and `noise`: {(quantity, L): the float32 restatement's largest error
    against the float64 oracle over the group's cases}."""

    def __init__(self, oracle):
        self.oracle, self.noise, self.worst = oracle, {}, {}
        self.cases = {s: W.Case(oracle, *s) for s in R.SWEEP}
        self.walk = {s: W.Case(oracle, *s, rows=(R.WALK_M, WALK_N), layouts=WALK_LAYOUTS) for s in R.WALK_SHAPES}
        for c in list(self.cases.values()) + list(self.walk.values()):
            for k, v in c.noise().items():
                key = (k, c.shape[2])
                self.noise[key] = max(v, self.noise.get(key, 0.0))
        self.both = {s: W.Case(oracle, *s) for s in R.BOTH}  # checked bit for bit: no part in the bars
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


def inverse(ws, c, Mz, Mp, N=None, **kw):
    lp, z0, sld = ws.wide_flow_stream_log_prob_raw(*dev(c, Mz, Mp, N), *c.shape, **(kw or ALL))
    return {k: v for k, v in (("lp", lp), ("z0", z0), ("sld", sld)) if v is not None}


def forward(ws, c, Mz, Mp, N=None):
    zf, sldf = ws.wide_flow_stream_forward_raw(*dev(c, Mz, Mp, N), *c.shape)
    return dict(zf=zf, sldf=sldf)


# ---- 1. the sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SWEEP, ids=W.case_id)
def test_sweep_through_the_abi(ws, sw, shape):
    """Every row layout, both directions, every output: one launch each."""
    c = sw.cases[shape]
    assert not lib.tnf_wide_flow_supported(*shape) and ws.wide_flow_stream_supported(*shape)
    for Mz, Mp, N in W.ROWS + W.LP_ONLY_ROWS:
        what = "%s (%d, %d, %d)" % (W.case_id(shape), Mz, Mp, N)
        with one_launch(1, 0):
            got = inverse(ws, c, Mz, Mp, N)
        sw.check(c, got, c.want(Mz, Mp, N), what)
        if (Mz, Mp, N) in W.ROWS:
            with one_launch(0, 1):
                got = forward(ws, c, Mz, Mp, N)
            sw.check(c, got, c.want(Mz, Mp, N), what)


# ---- 2. the resident kernel's bits -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.SHIPPED_TILES)
@pytest.mark.parametrize("shape", R.BOTH, ids=W.case_id)
def test_bit_identical_with_the_resident_kernel(ws, wf, sw, shape, T):
    """The per-tile arithmetic is the same code: lp, z0, sld, zf and sldf equal tnf_wide_flow_*'s bit for bit at every T."""
    c = sw.both[shape]
    for Mz, Mp, N in ((3, 3, 33), (3, 1, 33)):
        args = dev(c, Mz, Mp, N) + shape
        ref = wf.wide_flow_log_prob_raw(*args, **ALL) + wf.wide_flow_forward_raw(*args)
        with forced_tiles(ws, T), one_launch(1, 1):
            got = ws.wide_flow_stream_log_prob_raw(*args, **ALL) + ws.wide_flow_stream_forward_raw(*args)
        for k, a, b in zip(("lp", "z0", "sld", "zf", "sldf"), got, ref):
            assert torch.equal(a, b), (k, Mz, Mp, float((a - b).abs().max()))


# ---- 3. the group walk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", R.SHIPPED_TILES)
@pytest.mark.parametrize("shape", R.WALK_SHAPES, ids=W.case_id)
def test_group_walk(ws, sw, shape, T):
    """N = 2 * 128 T + 17: three groups, the last with one full tile and one row.  M = 129 (one parameter row each, and one
    shared row): the x-grid is clamped to one workgroup per row, which walks all three groups with the ring running on
    across them.  M = 1: three workgroups, one group each, every image a first build.  Row 0 must not tell the two apart."""
    c, N = sw.walk[shape], R.walk_N(T)
    assert R.groups(N, T) == 3 and R.grid_x(N, R.WALK_M, T) == 1 and R.grid_x(N, 1, T) == 3
    assert R.max_tiles(shape[0], shape[2], shape[3]) >= T
    with forced_tiles(ws, T):
        with one_launch(1, 1):
            one = dict(inverse(ws, c, 1, 1, N), **forward(ws, c, 1, 1, N))
        sw.check(c, one, c.want(1, 1, N), "walk %s T=%d M=1" % (W.case_id(shape), T))
        for Mz, Mp in WALK_LAYOUTS[:2]:
            with one_launch(1, 1):
                got = dict(inverse(ws, c, Mz, Mp, N), **forward(ws, c, Mz, Mp, N))
            sw.check(c, got, c.want(Mz, Mp, N), "walk %s T=%d (%d, %d)" % (W.case_id(shape), T, Mz, Mp))
            for k in got:  # the image built at a group's end is the image of a first build
                assert torch.equal(got[k][:1], one[k]), (k, Mz, Mp)


# ---- 4. subsets and guards ---------------------------------------------------------------------------------------------------
def _guarded(n, lead):
    buf = torch.full((n + lead + 9,), GUARD, device="cuda")
    return buf, buf[lead:lead + n]


@pytest.mark.parametrize("lead", [1, 4], ids=["4-byte", "16-byte"])
@pytest.mark.parametrize("shape", [(5, 9, 2, 17), (8, 2, 5, 64), (64, 4, 2, 64)], ids=W.case_id)
def test_subsets_rows_offsets_and_guards(ws, sw, shape, lead):
    """N in {1, 15, 16, 17}; a parameter row stride 7 floats longer than the row with NaNs behind each row; z and every
    output `lead` floats into a buffer aligned to 256 bytes -- lead = 1: 4-byte aligned rows, so that D % 8 == 0 must take
    the element accesses; lead = 4: 16-byte aligned, the float4 accesses -- with NaNs around z and guard values before and
    after every output; every subset of the outputs, with the buffers of the outputs not asked for left untouched."""
    c = sw.cases[shape]
    D, M, P = shape[0], 3, W.flow_params(*shape)
    mean, alpha = c.stat[0].cuda(), c.stat[1].cuda()
    pbuf = torch.full((M, P + 7), float("nan"))
    pbuf[:, :P] = c.inputs(M, M)[1]
    pbuf = pbuf.cuda()
    for N in (1, 15, 16, 17):
        z = c.inputs(M, M, N)[0]
        zbuf = torch.full((M * N * D + lead + 8,), float("nan"))
        zbuf[lead:lead + M * N * D] = z.reshape(-1)
        zin = zbuf.cuda()[lead:]
        assert zin.data_ptr() % 16 == (4 * lead) % 16
        want = c.want(M, M, N)
        dense = dict(inverse(ws, c, M, M, N), **forward(ws, c, M, M, N))
        for fwd, subsets in ((False, (("lp", "z", "sld"), ("lp",), ("z",), ("sld",), ("z", "sld"))),
                             (True, (("z", "sld"), ("z",), ("sld",)))):
            names = dict(z="zf", sld="sldf") if fwd else dict(lp="lp", z="z0", sld="sld")
            for asked in subsets:
                bufs = dict(lp=_guarded(M * N, lead), z=_guarded(M * N * D, lead), sld=_guarded(M * N, lead))
                ptr = {k: (v[1].data_ptr() if k in asked else None) for k, v in bufs.items()}
                with one_launch(int(not fwd), int(fwd)):
                    if fwd:
                        L_.check(lib.tnf_wide_flow_stream_forward_f32(
                            zin.data_ptr(), pbuf.data_ptr(), mean.data_ptr(), alpha.data_ptr(), ptr["z"], ptr["sld"], M, M, N,
                            *shape, P + 7, L_.stream_ptr()))
                    else:
                        L_.check(lib.tnf_wide_flow_stream_log_prob_f32(
                            zin.data_ptr(), pbuf.data_ptr(), mean.data_ptr(), alpha.data_ptr(), ptr["lp"], ptr["z"], ptr["sld"],
                            M, M, N, *shape, P + 7, L_.stream_ptr()))
                torch.cuda.synchronize()
                got = {}
                for k, (buf, view) in bufs.items():
                    if k not in asked:
                        assert bool((buf == GUARD).all()), "%s: not asked for, written" % k
                        continue
                    inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
                    inside[view.storage_offset():view.storage_offset() + view.numel()] = True
                    assert bool((buf[~inside] == GUARD).all()), "%s: a guard float changed" % names[k]
                    got[names[k]] = view.reshape((M, N, D) if k == "z" else (M, N)).clone()
                if len(asked) > 1:
                    sw.check(c, got, want, "offset %s N=%d lead=%d %s" % (W.case_id(shape), N, lead, "forward" if fwd else "inverse"))
                # the same bits as the aligned, densely packed call with every output
                assert all(torch.equal(got[k], dense[k]) for k in got), (asked, N)


# ---- 5. reproducibility and capture ---------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(ws, sw):
    for shape in ((33, 9, 1, 17), (64, 1, 3, 64), (5, 3, 4, 20)):
        c = sw.cases[shape]
        a, b = inverse(ws, c, 3, 3), inverse(ws, c, 3, 3)
        assert all(torch.equal(a[k], b[k]) for k in a)
        a, b = forward(ws, c, 3, 1), forward(ws, c, 3, 1)
        assert all(torch.equal(a[k], b[k]) for k in a)
    c = sw.walk[R.WALK_SHAPES[0]]
    a, b = inverse(ws, c, R.WALK_M, 1), inverse(ws, c, R.WALK_M, 1)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("shape", [(5, 9, 2, 17), (64, 2, 4, 33)], ids=W.case_id)
def test_log_prob_of_the_samples(ws, sw, shape):
    """log_prob(forward(omega)) against log N(omega) - sum_log_det of the float64 oracle.  Bar: 4 x the error of the same
    composition in the float32 restatement (its log_prob on its own forward's z) against the same float64 value."""
    c = sw.cases[shape]
    z, p, mean, alpha = dev(c, 3, 3)
    omega, params = c.inputs(3, 3)
    want = torch.tensor(sw.oracle.base_log_density_f64(omega.double().numpy())) - c.want(3, 3, W.N_FULL)["sldf"]
    with torch.no_grad():
        z32 = W.wide_flow_forward(omega, params, *shape, c.stat)[0]
        noise = W.err(W.wide_flow_log_prob(z32, params, *shape, c.stat)[0], want)
    zf, _ = ws.wide_flow_stream_forward_raw(z, p, mean, alpha, *shape)
    lp = ws.wide_flow_stream_log_prob_raw(zf, p, mean, alpha, *shape)[0]
    e = W.err(lp, want)
    print("round trip %s: err %.2e / bar %.2e" % (W.case_id(shape), e, 4 * noise))
    assert e <= 4 * noise


def test_graph_capture(ws, sw):
    """One log_prob call captured on a single stream (no parallel branches) replays to the same bits."""
    c = sw.cases[(33, 3, 2, 20)]
    args = dev(c, 3, 3) + c.shape
    eager = ws.wide_flow_stream_log_prob_raw(*args)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ws.wide_flow_stream_log_prob_raw(*args)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lp = ws.wide_flow_stream_log_prob_raw(*args)[0]
    before = stream_counts()
    lp.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert stream_counts() == before  # a replay runs the captured kernel; no call reaches the host launcher
    assert torch.equal(lp, eager)


class _nothing(object):
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ---- 6. through NormFlow and ConditionalDensityEstimator ----------------------------------------------------------------------------
def test_headline_model_with_64_units(tnf, sw, oracle):
    """NormFlow(64, False, 'coupling', 4, 2, 64) at N = 33: log_prob, inverse_and_log_det and sample are one launch of the
    new family each with the switch on; with it off the same calls run the wide per-layer chain (D % 8 == 0), and the two
    agree: both lie within the L = 2 bars of the float64 oracle, so within twice the bar of each other."""
    shape, N = R.NF_SHAPE, 33
    D = shape[0]
    c = sw.cases[shape]
    nf = tnf.NormFlow(D, False, "coupling", *shape[1:])
    assert (nf.num_stages, nf.num_layers, nf.num_units, nf.D_params) == shape[1:] + (W.flow_params(*shape),)
    assert nf.wide_flow_streamed is False
    nf.params = c.inputs(1, 1)[1].cuda()
    for i, b in enumerate(nf._bn_layers()):
        b.set_last_stats(c.stat[0][i], c.stat[1][i])
    z = c.inputs(1, 1)[0].cuda()
    want = c.want(1, 1, N)
    gen = torch.Generator(device="cuda").manual_seed(7)
    omega = torch.randn((1, N, D), device="cuda", dtype=torch.float32, generator=gen).cpu()
    with float64(), torch.no_grad():
        st = W.stats_list(c.stat, torch.float64)
        zs_w, lq_w, _ = oracle.flow_forward(omega.double().numpy(), c.inputs(1, 1)[1].double(), *shape, st)
    out = {}
    with torch.no_grad():
        for on in (False, True):
            nf.wide_flow_streamed = on
            mine, diag = stream_counts(), H.counts()
            with one_launch(1, 0) if on else _nothing():
                lp = nf.log_prob(z)
            with one_launch(1, 0) if on else _nothing():
                z0, sld = nf.inverse_and_log_det(z, nf.params)
            gen.manual_seed(7)
            with one_launch(0, 1) if on else _nothing():
                zs, lq = nf.sample(N, freeze_bn=True, generator=gen)
            assert lq.dtype == torch.float64
            if not on:  # today's route: the wide per-layer chain counts its launches, the new kernel never ran
                assert stream_counts() == mine and H.launched(diag).get(L_.DIAG_COUPLING_WIDE, 0) > 0
            out[on] = dict(lp=lp, z0=z0, sld=sld, zs=zs, lq=lq)
    sw.check(c, {k: out[True][k] for k in ("lp", "z0", "sld")}, want, "NormFlow %s" % W.case_id(shape))
    bars = dict(lp=sw.bar("lp", 2), z0=sw.bar("z0", 2), sld=sw.bar("sld", 2), zs=sw.bar("zf", 2), lq=sw.bar("sldf", 2))
    for k, w in (("zs", zs_w), ("lq", lq_w)):
        e = W.err(out[True][k], w)
        print("NormFlow sample %-2s err %.2e / bar %.2e" % (k, e, bars[k]))
        assert out[True][k].shape == w.shape and e <= bars[k], k
    for k in out[True]:
        ref = want.get(k, dict(zs=zs_w, lq=lq_w).get(k))
        e = W.err(out[True][k], out[False][k].double(), max(1.0, float(ref.abs().max())))
        print("on / off %-3s err %.2e / 2 bars %.2e" % (k, e, 2 * bars[k]))
        assert e <= 2 * bars[k], k


@pytest.mark.parametrize("support", [False, True], ids=["plain", "ToInterval"])
def test_conditional_estimator_calls(tnf, sw, oracle, support):
    """NormFlow(4, True, 'coupling', 5, 2, 20) inside a ConditionalDensityEstimator, the switch on: cde.log_prob(z (M, 33, 4),
    x) and cde.sample(x, 33) are one launch of the new kernel each -- with a ToInterval support layer too, which runs as
    its own kernel around it.  Reference (plain): the float64 oracle on float64 copies of the parameter rows the conditioner
    hands the flow.  Bars: the L = 2 groups, or 4 x the float32 restatement's error on these very inputs where that is larger
    (the rows follow the conditioner's law, not the sweep's).  With the support layer: the switch-off call, within twice
    those bars."""
    shape, M, N = R.CDE_SHAPE, 5, 33
    D = shape[0]
    torch.manual_seed(4)
    sup = tnf.ToInterval(D, [-1.0] * D, [2.0] * D) if support else None
    nf = tnf.NormFlow(D, True, "coupling", *shape[1:], support_layer=sup)
    cde = tnf.ConditionalDensityEstimator(nf, 8, [100])
    g = torch.Generator().manual_seed(4)
    for b in nf._bn_layers():
        b.set_last_stats(torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) * 0.5 + 0.75)
    with torch.no_grad():
        for q in cde.param_net.parameters():
            q.mul_(0.5)
    cde.cuda()
    assert (nf.num_units, nf.num_stages, nf.wide_flow_streamed) == (20, 5, False)
    x, z = torch.randn(M, 8, generator=g), torch.randn(M, N, D, generator=g)
    if support:
        z = torch.rand(M, N, D, generator=g) * 2.8 - 0.9  # inside the interval (-1, 2)
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

        mine, diag = stream_counts(), H.counts()
        lp_off = cde.log_prob(z.cuda(), x.cuda())
        gen.manual_seed(11)
        zs_off, lq_off = cde.sample(x.cuda(), N, generator=gen)
        assert stream_counts() == mine and H.launched(diag) == {}  # switch off: the composition, which has no counter
        nf.wide_flow_streamed = True
        with one_launch(1, 0):
            lp = cde.log_prob(z.cuda(), x.cuda())
        gen.manual_seed(11)
        with one_launch(0, 1):
            zs, lq = cde.sample(x.cuda(), N, generator=gen)
    got, off = dict(lp=lp, zf=zs, lq=lq), dict(lp=lp_off, zf=zs_off, lq=lq_off)
    for k in want:
        assert got[k].shape == want[k].shape
        if not support:
            e = W.err(got[k], want[k])
            print("cde %-2s err %.2e / bar %.2e" % (k, e, bars[k]))
            assert e <= bars[k], k
        e = W.err(got[k], off[k].double().cpu(), max(1.0, float(off[k].abs().max())))
        print("cde on / off %-2s err %.2e / 2 bars %.2e" % (k, e, 2 * bars[k]))
        assert e <= 2 * bars[k], k
