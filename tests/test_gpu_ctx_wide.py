"""Per-context coupling flows above 16 units with fewer than 32 samples per context, one launch per call each way
(include/tnf_ctxwide.h, csrc/flow_ctx_wide.hip, csrc/flow_ctx_wide_bwd.hip, NormFlow's families `context_rows_wide` and
`train_context_wide`) against the CPU oracle run in float64 on float64 copies of the same float32 inputs.  Inputs are
those of tests/test_gpu_ctx_flow.py (`inputs`), upstream gradients those of tests/test_gpu_ctx_train.py (`upstream`).

Inference bars.  Errors are maf_restatement.err (max |got - want| / max(1, max |want|)).  Each (quantity, L) group of the
sweep takes 4 x the largest error of the float32 restatement (tests/ctxwide_restatement.py) against float64 on the
sweep's own inputs: computed here from the restatement, never from the kernel.

Training bars.  BAR_P and BAR_Z of tests/domain_helpers.py, whole (conftest.grad_err) and per context row (`row_err`).
The float32 restatement of the walk alone stays within a quarter of them on every group but one
(tools/ctxwide_grad_restatement.py, profiles/r22_ctxwide_grad_errors.json): at S = 9, L = 1 the reversible rebuild through
18 one-hidden-layer couplings at D = 64, U >= 48 loses 6.5e-5 (parameters) and 5.0e-5 (z) in float32 arithmetic of any
order; that group takes 4 x the restatement's error, computed here (`group_bar`)."""
import collections

import numpy as np
import pytest
import torch

import ctxwide_restatement as R
import domain_helpers as H
import test_gpu_ctx_flow as CF
import test_gpu_ctx_train as CT
from conftest import grad_err
from domain_helpers import BAR_P, BAR_Z, float64
from maf_restatement import err
from test_gpu_ctx_flow import inputs, st64
from test_gpu_ctx_train import reference, row_err, upstream
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def cw(tnf):
    from torch_nf_amd import ctxwide_ops

    return ctxwide_ops


def wide_counts():
    torch.cuda.synchronize()
    return [lib.tnf_ctx_wide_launch_count(i) for i in range(3)]


def other_counts():
    return (CF.ctx_counts() + [lib.tnf_ctx_train_launch_count(), lib.tnf_ctx_sample_launch_count(),
                               lib.tnf_wide_flow_launch_count(0), lib.tnf_wide_flow_launch_count(1)])


class launches(object):
    """`with launches(lp, fwd, bwd)`: the block moves the three new counters by exactly that, and no other counter of the
    per-context and wide families and no diag family."""

    def __init__(self, lp, fwd, bwd):
        self.want = [lp, fwd, bwd]

    def __enter__(self):
        self.before, self.others, self.diag = wide_counts(), other_counts(), H.counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert [a - b for a, b in zip(wide_counts(), self.before)] == self.want
            assert other_counts() == self.others and H.launched(self.diag) == {}
        return False


class quiet(object):
    """`with quiet()`: the block moves none of the three new counters (today's routes may launch what they launch)."""

    def __enter__(self):
        self.before = wide_counts()

    def __exit__(self, *exc):
        if exc[0] is None:
            assert wide_counts() == self.before
        return False


def dev(*ts):
    return tuple(t.cuda() for t in ts)


# ---- inference: the sweep --------------------------------------------------------------------------------------------------
QUANTITIES = ("lp", "z0", "sld", "lp1", "zf", "sldf")  # lp1: log_prob with one block of z for every context


class Sweep(object):
    """Every case's inputs, float64 references and float32 restatement, once; `bars`: {(quantity, L): 4 x the group's
    largest restatement error}."""

    def __init__(self, oracle):
        self.cases, noise = {}, collections.defaultdict(float)
        for c in R.forward_cases():
            D, S, L, U, M, N = c
            params, mean, alpha, z = inputs(oracle, *c)
            z1 = inputs(oracle, *c, Mz=1)[3]
            shape, stat = (D, S, L, U), (mean, alpha)
            lp, z0, sld = CF.ref_inverse(oracle, z, params, mean, alpha, *shape)
            lp1 = CF.ref_inverse(oracle, z1.expand(M, N, D), params, mean, alpha, *shape)[0]
            zf, sldf, _ = CF.ref_forward(oracle, z, params, mean, alpha, *shape)
            want = dict(lp=lp, z0=z0, sld=sld, lp1=lp1, zf=zf, sldf=sldf)
            with torch.no_grad():
                r = R.ctx_wide_log_prob(z, params, *shape, stat)
                rf = R.ctx_wide_forward(z, params, *shape, stat)
                fold = dict(lp=r[0], z0=r[1], sld=r[2], lp1=R.ctx_wide_log_prob(z1, params, *shape, stat)[0], zf=rf[0],
                            sldf=rf[1])
            assert rf[2] == 0.0  # the padded slots of the restatement stay exactly 0
            for k in QUANTITIES:
                noise[(k, L)] = max(noise[(k, L)], err(fold[k], want[k]))
            self.cases[c] = (params, mean, alpha, z, z1, want)
        self.noise = dict(noise)
        self.bars = {k: 4.0 * v for k, v in noise.items()}
        assert all(0.0 < v < 1e-4 for v in self.bars.values()), self.bars


@pytest.fixture(scope="module")
def sweep(oracle):
    return Sweep(oracle)


@pytest.mark.parametrize("case", R.forward_cases(), ids=R.case_id)
def test_forward_domain(cw, sweep, case):
    """One shape per (HT, UT) cell at every depth, one and two tiles and their edges, several S: both directions through
    the C ABI, log_prob with one block of z per context and with one for all; one launch each."""
    D, S, L, U, M, N = case
    params, mean, alpha, z, z1, want = sweep.cases[case]
    shape = (D, S, L, U)
    p, mu, al = dev(params, mean, alpha)
    with launches(1, 0, 0):
        lp, z0, sld = cw.ctx_wide_log_prob_raw(z.cuda(), p, mu, al, *shape, want_lp=True, want_z0=True, want_sld=True)
    with launches(1, 0, 0):
        lp1 = cw.ctx_wide_log_prob_raw(z1.cuda(), p, mu, al, *shape)[0]
    with launches(0, 1, 0):
        zf, sldf = cw.ctx_wide_forward_raw(z.cuda(), p, mu, al, *shape)
    got = dict(lp=lp, z0=z0, sld=sld, lp1=lp1, zf=zf, sldf=sldf)
    bad = []
    for k in QUANTITIES:
        e, bar = err(got[k], want[k]), sweep.bars[(k, L)]
        print("ctx_wide %s %s: %.3e (bar %.3e, restatement %.3e)" % (R.case_id(case), k, e, bar, sweep.noise[(k, L)]))
        assert got[k].shape == want[k].shape
        if not e <= bar:
            bad.append((k, e, bar))
    assert not bad, bad


def test_subsets_of_the_outputs(cw, oracle):
    D, S, L, U, M, N = 33, 1, 2, 20, 3, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    d = dev(z, params, mean, alpha) + (D, S, L, U)
    full = cw.ctx_wide_log_prob_raw(*d, want_lp=True, want_z0=True, want_sld=True)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, True, True), (True, True, False),
                 (True, False, True)):
        with launches(1, 0, 0):
            got = cw.ctx_wide_log_prob_raw(*d, want_lp=want[0], want_z0=want[1], want_sld=want[2])
        for w, a, b in zip(want, got, full):
            assert (a is None) if not w else torch.equal(a, b)
    # the sampling entry through the C ABI: z_out alone, sum_log_det alone
    zf, sldf = cw.ctx_wide_forward_raw(*d)
    P = params.shape[1]
    for want_z, want_s in ((True, False), (False, True)):
        zo = torch.full((M, N, D), 7.0, device="cuda") if want_z else None
        so = torch.full((M, N), 7.0, device="cuda") if want_s else None
        with launches(0, 1, 0):
            rc = lib.tnf_ctx_wide_forward_f32(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                              zo.data_ptr() if want_z else None, so.data_ptr() if want_s else None, M, N, D,
                                              S, L, U, P, L_.stream_ptr())
        assert rc == 0
        assert torch.equal(zo, zf) if want_z else torch.equal(so, sldf)


def test_rows_stay_with_their_contexts_and_runs_repeat(cw, oracle):
    """Context m's outputs and gradient row are those of a call with that context alone, bit for bit; a permutation of the
    contexts permutes them; two runs give the same bits."""
    D, S, L, U, M, N = 6, 2, 2, 20, 6, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, seed=3)
    assert len({tuple(r.tolist()) for r in params}) == M  # pairwise different rows
    g, shape = upstream(M, N), (D, S, L, U)
    mu, al = dev(mean, alpha)

    def run(z, params, g):
        zc, pc, gc = dev(z, params, g)
        inv = cw.ctx_wide_log_prob_raw(zc, pc, mu, al, *shape, want_lp=True, want_z0=True, want_sld=True)
        fwd = cw.ctx_wide_forward_raw(zc, pc, mu, al, *shape)
        bwd = cw.ctx_wide_log_prob_bwd_raw(inv[1], pc, mu, al, gc, *shape)
        return inv + fwd + bwd

    got = run(z, params, g)
    for a, b in zip(got, run(z, params, g)):
        assert torch.equal(a, b)
    for m in range(M):
        for a, b in zip(got, run(z[m:m + 1], params[m:m + 1], g[m:m + 1])):
            assert torch.equal(a[m:m + 1], b), m
    perm = torch.tensor([4, 0, 5, 2, 1, 3])
    for a, b in zip(got, run(z[perm], params[perm], g[perm])):
        assert torch.equal(a[perm.cuda()], b)


def test_alignment_strides_and_guards(cw, oracle):
    """Rows at 4-byte alignment (every buffer one float off a 16-byte boundary), a parameter and a gradient row stride
    beyond the row with NaN behind the row, and guard values around every output: all intact, same bits as the plain call."""
    D, S, L, U, M, N = 7, 2, 2, 20, 5, 17
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    g, shape = upstream(M, N), (D, S, L, U)
    P, pad = params.shape[1], 7
    zc, pc, mu, al, gc = dev(z, params, mean, alpha, g)
    lp, z0, sld = cw.ctx_wide_log_prob_raw(zc, pc, mu, al, *shape, want_lp=True, want_z0=True, want_sld=True)
    zf, sldf = cw.ctx_wide_forward_raw(zc, pc, mu, al, *shape)
    gp, gz = cw.ctx_wide_log_prob_bwd_raw(z0, pc, mu, al, gc, *shape)

    def off(t, cols=None):
        """A copy of t one float past a 16-byte boundary with guards around it -> (view, buffer, slice of the view)."""
        n = t.numel() if cols is None else t.shape[0] * cols
        buf = torch.full((n + 9,), float("nan"), device="cuda")
        if cols is None:
            view = buf[5:5 + n].view(t.shape)
        else:
            view = buf[5:5 + n].view(t.shape[0], cols)[:, :t.shape[1]]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view, buf

    def guards_intact(buf, view, cols=None):
        inside = torch.zeros_like(buf, dtype=torch.bool)
        n = view.numel() if cols is None else view.shape[0] * cols
        region = inside[5:5 + n]
        if cols is None:
            region[:] = True
        else:
            region.view(view.shape[0], cols)[:, :view.shape[1]] = True
        return bool(torch.isnan(buf[~inside]).all()) and not bool(torch.isnan(buf[inside]).any())

    z_v, _ = off(zc)
    p_v, _ = off(pc, cols=P + pad)  # pstride = P + 7, NaN behind every row
    mu_v, _ = off(mu)
    al_v, _ = off(al)
    g_v, _ = off(gc)
    outs = {k: off(torch.zeros_like(t)) for k, t in (("lp", lp), ("z0", z0), ("sld", sld), ("zf", zf), ("sldf", sldf), ("gz", gz))}
    gp_v, gp_buf = off(torch.zeros_like(gp), cols=P + pad)
    gp_buf[:] = float("nan")  # gradient rows need no initialisation; columns beyond P are not touched
    st = L_.stream_ptr()
    with launches(1, 1, 1):
        assert lib.tnf_ctx_wide_log_prob_f32(z_v.data_ptr(), p_v.data_ptr(), mu_v.data_ptr(), al_v.data_ptr(),
                                             outs["lp"][0].data_ptr(), outs["z0"][0].data_ptr(), outs["sld"][0].data_ptr(),
                                             M, M, N, D, S, L, U, P + pad, st) == 0
        assert lib.tnf_ctx_wide_forward_f32(z_v.data_ptr(), p_v.data_ptr(), mu_v.data_ptr(), al_v.data_ptr(),
                                            outs["zf"][0].data_ptr(), outs["sldf"][0].data_ptr(), M, N, D, S, L, U, P + pad,
                                            st) == 0
        assert lib.tnf_ctx_wide_log_prob_bwd_f32(outs["z0"][0].data_ptr(), p_v.data_ptr(), mu_v.data_ptr(), al_v.data_ptr(),
                                                 g_v.data_ptr(), gp_v.data_ptr(), outs["gz"][0].data_ptr(), M, N, D, S, L, U,
                                                 P + pad, P + pad, st) == 0
    for k, want in (("lp", lp), ("z0", z0), ("sld", sld), ("zf", zf), ("sldf", sldf), ("gz", gz)):
        view, buf = outs[k]
        assert torch.equal(view, want), k
        assert guards_intact(buf, view), k
    assert torch.equal(gp_v, gp) and guards_intact(gp_buf, gp_v, cols=P + pad)


def test_closed_launch_gate_leaves_the_outputs_untouched(cw, oracle):
    D, S, L, U, M, N = 5, 2, 2, 20, 3, 9
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N)
    zc, pc, mu, al, gc = dev(z, params, mean, alpha, upstream(M, N))
    P, st = params.shape[1], L_.stream_ptr()
    gate = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = [torch.full(s, 7.0, device="cuda") for s in ((M, N), (M, N, D), (M, N), (M, N, D), (M, N), (M, P), (M, N, D))]
    z0 = cw.ctx_wide_log_prob_raw(zc, pc, mu, al, D, S, L, U, want_lp=False, want_z0=True)[1]

    def calls():
        assert lib.tnf_ctx_wide_log_prob_f32(zc.data_ptr(), pc.data_ptr(), mu.data_ptr(), al.data_ptr(), outs[0].data_ptr(),
                                             outs[1].data_ptr(), outs[2].data_ptr(), M, M, N, D, S, L, U, P, st) == 0
        assert lib.tnf_ctx_wide_forward_f32(zc.data_ptr(), pc.data_ptr(), mu.data_ptr(), al.data_ptr(), outs[3].data_ptr(),
                                            outs[4].data_ptr(), M, N, D, S, L, U, P, st) == 0
        assert lib.tnf_ctx_wide_log_prob_bwd_f32(z0.data_ptr(), pc.data_ptr(), mu.data_ptr(), al.data_ptr(), gc.data_ptr(),
                                                 outs[5].data_ptr(), outs[6].data_ptr(), M, N, D, S, L, U, P, P, st) == 0

    assert lib.tnf_set_launch_gate(gate.data_ptr()) == 0
    try:
        with launches(1, 1, 1):  # the calls reach their launches; the kernels return at once
            calls()
        assert all(bool((o == 7.0).all()) for o in outs)
        gate.fill_(1)
        calls()
        torch.cuda.synchronize()
    finally:
        assert lib.tnf_set_launch_gate(None) == 0
    assert not any(bool((o == 7.0).all()) for o in outs)
    assert torch.equal(outs[1], z0)


def test_no_samples_no_launch(cw, oracle):
    D, S, L, U, M = 5, 2, 2, 20, 3
    params, mean, alpha, _ = inputs(oracle, D, S, L, U, M, 8)
    p, mu, al = dev(params, mean, alpha)
    with launches(0, 0, 0):
        gp, gz = cw.ctx_wide_log_prob_bwd_raw(torch.zeros(M, 0, D).cuda(), p, mu, al, torch.zeros(M, 0).cuda(), D, S, L, U)
    assert gp.shape == params.shape and not gp.any() and gz.shape == (M, 0, D)


# ---- training ------------------------------------------------------------------------------------------------------------
WIDTHS, SAMPLES = (2, 5, 16, 31, 32, 33, 63, 64), (1, 2, 15, 16, 17, 31)
LARGEST = (64, 1, 2, 64, 2, 31)  # the largest slice at L <= 2: 123,008 bytes


def train_groups():
    """{group: [(D, S, L, U, M, N)]}: the training cases, in the groups that share a bar."""
    out = collections.OrderedDict()
    out["widths_and_samples"] = [(D, 2, 2, 20, 5, N) for D in WIDTHS for N in SAMPLES]
    for S in (1, 9):
        for L in (1, 3):
            out["depth_and_units S=%d L=%d" % (S, L)] = [(D, S, L, U, 3, 7) for D in (5, 64) for U in (17, 48, 64)]
    out["largest_slice"] = [LARGEST]
    return out


def group_bar(bar, restatement):
    """The group's bar: the suite's, unless the float32 restatement alone exceeds a quarter of it -- then 4 x its error."""
    return bar if restatement <= bar / 4 else 4.0 * restatement


def restatement_grad_errors(oracle, case):
    """{"params", "z"}: the float32 restatement of forward and walk against float64 autograd, the larger of the whole and
    the per-row error."""
    D, S, L, U, M, N = case
    params, mean, alpha, z = inputs(oracle, *case)
    g = upstream(M, N)
    want = reference(oracle, z, params, mean, alpha, g, (D, S, L, U), key=case)
    with torch.no_grad():
        z0 = R.ctx_wide_log_prob(z, params, D, S, L, U, (mean, alpha))[1]
        gp, gz = R.ctx_wide_log_prob_bwd(z0, params, (mean, alpha), g, D, S, L, U)
    return {"params": max(grad_err("ctxwide restatement params", gp, want[0]), row_err(gp, want[0])),
            "z": max(grad_err("ctxwide restatement z", gz, want[1]), row_err(gz, want[1]))}


_GROUP_BARS = {}


def depth_bars(oracle, S, L):
    """(bar for params, bar for z) of a depth_and_units group, from the restatement on the group's own cases."""
    if (S, L) not in _GROUP_BARS:
        errs = [restatement_grad_errors(oracle, c) for c in train_groups()["depth_and_units S=%d L=%d" % (S, L)]]
        _GROUP_BARS[(S, L)] = (group_bar(BAR_P, max(e["params"] for e in errs)), group_bar(BAR_Z, max(e["z"] for e in errs)))
    return _GROUP_BARS[(S, L)]


def check(tag, gp, gz, want, bars=(BAR_P, BAR_Z)):
    for name, got, ref, bar in (("params", gp, want[0], bars[0]), ("z", gz, want[1], bars[1])):
        if got is None:
            continue
        whole, rows = grad_err("ctx_wide %s %s" % (tag, name), got, ref), row_err(got, ref)
        print("ctx_wide %s %s: whole %.3e per row %.3e (bar %.1e)" % (tag, name, whole, rows, bar))
        assert whole <= bar and rows <= bar, (tag, name, whole, rows, bar)


def step(cw, z, params, mean, alpha, g, shape, z_grad=True):
    """One forward + backward through the autograd entry on the device -> (log_prob, g_params, g_z | None)."""
    pc, zc = params.cuda().requires_grad_(), z.cuda().requires_grad_(z_grad)
    lp = cw.ctx_wide_log_prob_train(zc, pc, mean.cuda(), alpha.cuda(), *shape)
    lp.backward(g.cuda())
    return lp.detach(), pc.grad, zc.grad


def train_case(cw, oracle, case, bars=(BAR_P, BAR_Z)):
    D, S, L, U, M, N = case
    params, mean, alpha, z = inputs(oracle, *case)
    g, shape = upstream(M, N), (D, S, L, U)
    with launches(1, 0, 1):
        _, gp, gz = step(cw, z, params, mean, alpha, g, shape)
    assert gp.shape == params.shape and gz.shape == z.shape
    check(R.case_id(case), gp, gz, reference(oracle, z, params, mean, alpha, g, shape, key=case), bars)


@pytest.mark.parametrize("N", SAMPLES)
@pytest.mark.parametrize("D", WIDTHS)
def test_widths_and_samples(cw, oracle, D, N):
    """Both parities of D, h = 1, the widths on either side of 32, one sample, 16 and its neighbours, 31."""
    train_case(cw, oracle, (D, 2, 2, 20, 5, N))


@pytest.mark.parametrize("S", [1, 9])
@pytest.mark.parametrize("D", [5, 64])
@pytest.mark.parametrize("U", [17, 48, 64])
@pytest.mark.parametrize("L", [1, 3])
def test_depth_and_units(cw, oracle, L, U, D, S):
    train_case(cw, oracle, (D, S, L, U, 3, 7), depth_bars(oracle, S, L))


def test_largest_slice(cw, oracle):
    assert cw.lds_bytes(cw.LDS_BACKWARD, *LARGEST[:4], LARGEST[5]) == 123008
    train_case(cw, oracle, LARGEST)


def test_outputs_requested(cw, oracle):
    """g_z is None when z does not require grad; a shared block z (1, N, D) that requires no grad runs the pair and matches
    the oracle on the expanded z."""
    D, S, L, U, M, N = 5, 2, 2, 20, 5, 9
    params, mean, alpha, z = inputs(oracle, D, S, L, U, M, N, Mz=1)
    assert z.shape[0] == 1
    g, shape = upstream(M, N), (D, S, L, U)
    with launches(1, 0, 1):
        lp, gp, gz = step(cw, z, params, mean, alpha, g, shape, z_grad=False)
    assert gz is None and lp.shape == (M, N)
    check("shared z", gp, None, reference(oracle, z.expand(M, N, D).contiguous(), params, mean, alpha, g, shape))
    full = inputs(oracle, D, S, L, U, M, N)[3]
    _, gp_a, gz_a = step(cw, full, params, mean, alpha, g, shape)
    _, gp_b, gz_b = step(cw, full, params, mean, alpha, g, shape, z_grad=False)
    assert gz_b is None and gz_a is not None and torch.equal(gp_a, gp_b)
    check("z with grad", gp_a, gz_a, reference(oracle, full, params, mean, alpha, g, shape))


# ---- through NormFlow and ConditionalDensityEstimator ---------------------------------------------------------------
def make_nf(tnf, oracle, D, S, L, U, M, N, rows=True, training=True):
    nf, params, mean, alpha, z = CF.make_nf(tnf, oracle, D, S, L, U, M, N)
    nf.context_rows = False
    nf.wide_context_rows, nf.wide_context_training = rows, training
    return nf, params, mean, alpha, z


def test_the_reference_conditional_flow(tnf, oracle):
    """NormFlow(4, True, 'coupling', 1, 2, 20) with N = 1 per context, as the reference's train_SNPE evaluates
    cde.log_prob(z[:, None, :], x): one launch forward, one backward."""
    D, S, L, U, M, N = R.CDE_SHAPE + (6, 1)
    nf, params, mean, alpha, z = make_nf(tnf, oracle, D, S, L, U, M, N)
    want = CF.ref_inverse(oracle, z, params, mean, alpha, D, S, L, U)
    with torch.no_grad(), launches(2, 0, 0):
        lp = nf.log_prob(z.cuda(), params.cuda())
        z0, sld = nf.inverse_and_log_det(z.cuda(), params.cuda())
    CF.check_inverse((lp, z0, sld), want)
    pc = params.cuda().requires_grad_()
    with launches(1, 0, 1):
        out = nf.log_prob(z.cuda(), pc)
        (-out.mean()).backward()
    torch.testing.assert_close(out.detach(), lp, rtol=0, atol=0)
    ref = reference(oracle, z, params, mean, alpha, torch.full((M, N), -1.0 / (M * N)), (D, S, L, U))
    check("reference cde shape", pc.grad, None, ref)


@pytest.mark.parametrize("U", [20, 64])
def test_conditional_estimator_calls(tnf, oracle, U):
    """cde.log_prob(z (M, 8, D), x), cde(x, N = 8, freeze_bn=True), cde.sample(x, 8) and the backward of
    -cde.log_prob(z, x).mean(): each one launch of the new kernels per direction and no other flow kernel; against the
    float64 oracle on the materialised parameter rows, and with the switches off none of the new counters moves."""
    D, S, L, M, N = 5, 2, 2, 6, 8
    nf, cde = H._cde(tnf, D, S, L, 32, seed=U, U=U)
    g = torch.Generator().manual_seed(U)
    x = torch.randn(M, 8, generator=g)
    z = torch.randn(M, N, D, generator=g)
    up = upstream(M, N)
    shape = (D, S, L, U)

    def grads():
        cde.param_net.zero_grad(set_to_none=True)
        (cde.log_prob(z.cuda(), x.cuda()) * up.cuda()).sum().backward()
        return [p.grad.clone() for p in cde.param_net.parameters()]

    with quiet():  # the switches default to off: today's routes
        with torch.no_grad():
            lp_off = cde.log_prob(z.cuda(), x.cuda())
            np.random.seed(7)
            zs_off, lq_off = cde(x.cuda(), N=N, freeze_bn=True)
        off = grads()
    nf.wide_context_rows = nf.wide_context_training = True
    with float64():
        params64 = H._net64(cde)(x.double()).detach()
    stats = H._stats64_of(nf)
    with torch.no_grad():
        with launches(1, 0, 0):
            lp = cde.log_prob(z.cuda(), x.cuda())
        with float64():
            want = oracle.flow_log_prob(z.double(), params64, *shape, stats)
        torch.testing.assert_close(lp.cpu().double(), want, **H.LOGP_TOL)
        torch.testing.assert_close(lp, lp_off, **H.LOGP_TOL)
        np.random.seed(7)
        with launches(0, 1, 0):
            zs, lq = cde(x.cuda(), N=N, freeze_bn=True)
        np.random.seed(7)
        omega = np.random.normal(0.0, 1.0, (M, N, D))
        with float64():
            z_w, lq_w, _ = oracle.flow_forward(omega, params64, *shape, stats)
        torch.testing.assert_close(zs.cpu().double(), z_w, **H.ZF_TOL)
        torch.testing.assert_close(lq.cpu(), lq_w, **H.LQ_TOL)
        torch.testing.assert_close(zs, zs_off, **H.ZF_TOL)
        torch.testing.assert_close(lq, lq_off, **H.LQ_TOL)
        gen = torch.Generator(device="cuda").manual_seed(11)
        with launches(0, 1, 0):
            zs, lq = cde.sample(x.cuda(), N, generator=gen)
        gen.manual_seed(11)
        omega = torch.randn((M, N, D), device="cuda", dtype=torch.float32, generator=gen).cpu()
        with float64():
            z_w, lq_w, _ = oracle.flow_forward(omega.double().numpy(), params64, *shape, stats)
        torch.testing.assert_close(zs.cpu().double(), z_w, **H.ZF_TOL)
        torch.testing.assert_close(lq.cpu(), lq_w, **H.LQ_TOL)
    with launches(1, 0, 1):
        on = grads()
    net64 = H._net64(cde)
    with float64():
        (oracle.flow_log_prob(z.double(), net64(x.double()), *shape, stats) * up.double()).sum().backward()
    for i, (a, b, w) in enumerate(zip(on, off, net64.parameters())):
        e_today, e_ref = grad_err("ctx_wide cde U=%d p%d vs today" % (U, i), a, b), grad_err(
            "ctx_wide cde U=%d p%d vs float64" % (U, i), a, w.grad)
        print("ctx_wide cde U=%d param %d: vs today's route %.3e, vs float64 %.3e" % (U, i, e_today, e_ref))
        assert e_today <= BAR_P and e_ref <= BAR_P


def test_round_trip(tnf, oracle):
    """The sampling forward, then inverse_and_log_det: the draw comes back and the two log-dets agree."""
    D, S, L, U, M, N = 33, 2, 2, 48, 5, 17
    nf, params, mean, alpha, omega = make_nf(tnf, oracle, D, S, L, U, M, N)
    with torch.no_grad(), launches(1, 1, 0):
        z, log_q = nf._forward_from(omega.cuda(), params.cuda(), freeze_bn=True)
        back, sld = nf.inverse_and_log_det(z, params.cuda())
    torch.testing.assert_close(back.cpu(), omega, **H.INV_TOL)
    base = tnf.ops.base_log_density_f64(omega.cuda())
    torch.testing.assert_close((base - log_q).float(), sld, **H.INV_TOL)


def test_support_layer_runs_as_its_own_kernel(tnf, oracle):
    D, S, L, U, M, N = 5, 2, 2, 20, 5, 8
    lb, ub = -2.0 * np.ones(D), 3.0 * np.ones(D)
    nf, params, mean, alpha, _ = CF.make_nf(tnf, oracle, D, S, L, U, M, N, support=tnf.ToInterval(D, lb, ub))
    nf.context_rows = False
    nf.wide_context_rows = nf.wide_context_training = True
    z = torch.from_numpy(np.random.RandomState(0).uniform(-1.5, 2.5, (M, N, D)).astype(np.float32))
    g = upstream(M, N)
    consts = tuple(c.double() for c in oracle.interval_consts(lb, ub))
    before = wide_counts()
    pc, zc = params.cuda().requires_grad_(), z.cuda().requires_grad_()
    nf.log_prob(zc, pc).backward(g.cuda())
    with torch.no_grad():
        lp = nf.log_prob(z.cuda(), params.cuda())
        nf.inverse_and_log_det(z.cuda(), params.cuda())  # with a support layer: always the bijectors
    assert [a - b for a, b in zip(wide_counts(), before)] == [2, 0, 1]
    with float64():
        p64, z64 = params.double().requires_grad_(), z.double().requires_grad_()
        z_in, ld_sup = oracle.to_interval(z64, consts, True)
        want = oracle.flow_log_prob(z_in, p64, D, S, L, U, st64(mean, alpha)) - ld_sup
        (want * g.double()).sum().backward()
    torch.testing.assert_close(lp.cpu().double(), want.detach(), **H.LOGP_TOL)
    check("support layer", pc.grad, zc.grad, (p64.grad, z64.grad))


def test_other_calls_keep_their_routes(tnf, oracle):
    """Switches off, N = 32, U = 16, or the switch of the other direction alone: the new counters do not move and the
    results are today's, bit for bit."""
    D, S, L, U, M = 5, 2, 2, 20, 5
    nf, params, mean, alpha, _ = make_nf(tnf, oracle, D, S, L, U, M, 32)
    z = inputs(oracle, D, S, L, U, M, 32)[3].cuda()
    g = upstream(M, 32).cuda()
    pc = params.cuda()

    def both(rows, training, fn):
        keep = nf.wide_context_rows, nf.wide_context_training
        nf.wide_context_rows, nf.wide_context_training = rows, training
        try:
            return fn()
        finally:
            nf.wide_context_rows, nf.wide_context_training = keep

    def train(zz, gg):
        pg = pc.clone().requires_grad_()
        lp = nf.log_prob(zz, pg)
        lp.backward(gg)
        return lp.detach(), pg.grad

    with quiet():
        with torch.no_grad():
            off = both(False, False, lambda: nf.log_prob(z[:, :8], pc))
            assert torch.equal(both(False, True, lambda: nf.log_prob(z[:, :8], pc)), off)  # training switch alone
            assert torch.equal(nf.log_prob(z, pc), both(False, False, lambda: nf.log_prob(z, pc)))  # N = 32
            zs, lq = nf._forward_from(np.zeros((M, 32, D)), pc, freeze_bn=True)
            zs_t, lq_t = both(False, False, lambda: nf._forward_from(np.zeros((M, 32, D)), pc, freeze_bn=True))
            assert torch.equal(zs, zs_t) and torch.equal(lq, lq_t)
        t_off = both(False, False, lambda: train(z[:, :8], g[:, :8]))
        for a, b in zip(both(True, False, lambda: train(z[:, :8], g[:, :8])), t_off):  # inference switch alone
            assert torch.equal(a, b)
        for a, b in zip(train(z, g), both(False, False, lambda: train(z, g))):  # N = 32
            assert torch.equal(a, b)
    with torch.no_grad(), launches(1, 0, 0):
        on = nf.log_prob(z[:, :8], pc)
    torch.testing.assert_close(on, off, **H.LOGP_TOL)
    with launches(1, 0, 1):
        lp_on, gp_on = train(z[:, :8], g[:, :8])
    torch.testing.assert_close(lp_on, t_off[0], **H.LOGP_TOL)
    grad_err("ctx_wide vs today's route params", gp_on, t_off[1], BAR_P)
    # 16 units: the 16-unit families, never the new ones
    n16, p16, _, _, z16 = make_nf(tnf, oracle, D, S, L, 16, M, 8)
    n16.context_rows = n16.context_training = True
    before = CT.counters()
    with quiet():
        with torch.no_grad():
            n16.log_prob(z16.cuda(), p16.cuda())
        n16.log_prob(z16.cuda(), p16.cuda().requires_grad_()).sum().backward()
    assert [a - b for a, b in zip(CT.counters(), before)] == [2, 0, 1]


def test_graph_capture(tnf, oracle):
    """A whole step -- forward, backward, into preallocated .grad -- captured on a single stream (no parallel branches)
    replays to the eager step's bits; the counters do not move on replay."""
    D, S, L, U, M, N = 6, 2, 2, 20, 7, 8
    nf, params, mean, alpha, z = make_nf(tnf, oracle, D, S, L, U, M, N)
    g = upstream(M, N).cuda()
    pc, zc = params.cuda().requires_grad_(), z.cuda()
    pc.grad = torch.zeros_like(pc)

    def one_step():
        pc.grad.zero_()
        lp = nf.log_prob(zc, pc)
        lp.backward(g)
        return lp.detach()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up on the side stream
            one_step()
    torch.cuda.current_stream().wait_stream(s)
    lp_eager, gp_eager = one_step().clone(), pc.grad.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lp = one_step()
    before = wide_counts()
    pc.grad.fill_(7.0)
    lp.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert wide_counts() == before  # a replay runs the captured kernels; no call reaches the host launchers
    assert torch.equal(lp, lp_eager) and torch.equal(pc.grad, gp_eager)
