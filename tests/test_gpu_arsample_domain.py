"""maf_sample_bwd_kernel (csrc/maf_sample_bwd.hip) -- the one-launch backward of MAF.forward_and_log_det and of the frozen
[MAF, BatchNorm, Affine] stack -- over its own domain against float64, in the pattern of tests/test_gpu_maf_domain.py.
Restatement, grid, inputs and noise: tests/arsample_restatement.py (R) on the helpers of tests/maf_restatement.py (MR);
the host half, which pins the restatement to float64 autograd, counts the grid and plants the defects:
tests/test_arsample_host.py.  tests/test_gpu_arsample.py (seven shapes, bars from the switch-off route) stays as it is.

Reference: the float64 restatement on float64 copies of the same float32 inputs.  Every input is built on the CPU -- masks
by the package's rule, weights ~ N(0, MR.weight_scale(U)), omega ~ N(0, 1), x (z) = float32 of the float64 oracle's
sampling pass (stack forward), cotangents ~ N(0, 1), frozen statistics mean ~ N(0, 0.3), alpha ~ U(0.5, 1.5), Affine
a, b ~ N(0, 0.2) -- so no kernel output enters a reference.  Error: MR.gerr, conftest.grad_err's measure.

Bars.  The bar of a group (quantity, L) is 4 x the largest error in the group of the kernel's formulation restated in
float32 (R.maf_sample_bwd / R.ar_flow_sample_bwd with folded=True: r = 1 / (1 + 2^a), folded weights, column-sum seeds,
alpha in log2 units, h = 1 - 2 r, tanh' = 4 r (1 - r)) against that reference: room for another summation order and
1-ulp exp2 / rcp, not for a lower precision class.  Every bar but (f)'s is asserted to stay within CAP = 2e-4, the bound of
tests/test_gpu_arsample.py.  Every output must be finite.  No bar comes from a kernel's output.

a  tnf_maf_sample_bwd_f32 (arsample_ops.maf_sample_bwd_raw): the 40 supported shapes of MR.backward_cases() -- every
   (DT, UT, VEC, L) cell, 12 of them with one shared accumulator copy (the id names nacc) -- x MR.BWD_ROWS; g_omega and
   g_params, one `arsample` launch and no diag family moving, masked weights exactly zero, and on private-copy cells
   with per-context rows two runs bit-identical (on shared-copy cells the LDS float adds of the four waves are unordered
   once N > 16: the bar only).
b  Argument paths on R.ARG_CELLS (private / shared copy x VEC / non-VEC): g_x = None against explicit zeros, g_ld
   likewise, want_omega = False, a parameter block viewed out of a wider buffer with NaN behind each row -- bit for bit
   on the private-copy cells with per-context rows, under the bar on all; N = 1, 15, 16, 17; (130, 130, 3) and
   (130, 1, 3); g_params prefilled with 1.0 through ctypes (what "accumulated" means, see include/tnf_arsample.h); x and
   g_x 4 bytes past a 16-byte boundary at D = 16 (the launcher then takes the non-VEC instantiation).
c  tnf_ar_flow_sample_bwd_f32 (arsample_ops.ar_flow_sample_bwd_raw): the 20 supported shapes of MR.train_cases() x
   (3, 3, 37), (3, 1, 147) x both cotangents, g_z alone (g_sld None), g_sld alone; MAF block and Affine slice in groups
   of their own.
d  MR.LONG_CELLS at N = 32,789, one shared row: the 512-workgroup cap binds, a wave walks a second tile; both accumulator
   schemes; the bar from the restatement in 16-row tiles added in tile order in float32.
e  NormFlow(D, True, "AR", 1, L, U), ar_sample_training = True, frozen statistics, one shape per (DT, UT) of (c): route
   ar_train_sample, z and log_q bit-identical to the inference route, d/d params of sum(z w_z) + sum(log_q w_l) against
   float64 autograd from omega.  A kernel forward sits in front, so the group is its own: the float32 folded forward
   (MR.folded_ar_forward) pushed through the float32 folded backward, on the CPU.
f  Weights 0.05, L = 3 (MR.SMALL_WEIGHT): a group of its own, not capped (see test_small_weights).
g  The 8 refused shapes of MR.backward_cases(), D = 33 and L = 4: with MAF.fused_sampling_backward = True the backward is
   the switch-off composition (the `arsample` counter stays, a MAF backward family moves), held to CAP, the bound that
   composition has in tests/test_gpu_arsample.py and tests/test_gpu_maf.py.

Noise of each group (quantity, L) -- the folded restatement in float32 against the float64 restatement on the sweep's
inputs, as the CPU computed it where the host half was written (each run recomputes and prints it with the bar when a
section is built).  The bar is 4 x the entry.
  quantity                 L=1      L=2      L=3
  maf g_omega              8.2e-07  1.2e-06  8.4e-07
  maf g_params             1.1e-06  3.7e-06  5.0e-06
  args-1row g_omega        2.6e-07  2.7e-07  -
  args-1row g_params       1.9e-07  1.0e-05  -
  args-tile g_omega        7.2e-07  1.0e-06  -
  args-tile g_params       3.5e-07  1.1e-06  -
  args-130 g_omega         4.8e-07  7.6e-07  -
  args-130 g_params        5.9e-07  8.7e-07  -
  flow g_maf              5.8e-07  1.1e-06  2.9e-06
  flow g_affine            2.8e-06  2.4e-07  1.9e-06
  long g_omega             -        5.8e-07  -
  long g_params            -        1.6e-06  -
  nf g_maf                 6.4e-07  2.2e-06  2.2e-06
  nf g_affine              4.0e-07  4.7e-07  1.6e-06
  small-weight g_omega     -        -        8.4e-08
  small-weight g_params    -        -        9.8e-06
The largest entries are sums that nearly cancel, not a lower precision: maf g_params at D = 2 (two features, 37 rows);
args-1row g_params L = 2 at (2, 2, 48), a "sum" of one row, which is why the row layouts of (b) are groups by kind of
layout (R.arg_group); flow g_affine L = 1 at (28, 1, 33) with g_sld alone, where the whole slice is GS = sum g_sld --
pairwise sums understate the float32 noise of such a sum, which is why R._fold_sum adds the fold sums in the kernel's order.
Largest error / bar per group on the MI355X (the module prints each case's, and these when it is done):
maf g_omega 0.31, g_params 0.47; args-1row 0.35, 0.34; args-tile 0.30, 0.24; args-130 0.39, 0.22; flow g_maf 0.21,
g_affine 0.44; long g_omega 0.31, g_params 0.12 .. 0.17 over three runs (the shared row's atomics move it); nf g_maf
0.31, g_affine 0.20; small-weight g_omega 0.32, g_params 0.24; refused shapes at most 8.5e-7 against CAP.  Nothing
exceeded its bar; every bit-identity asserted held.
Module time on the MI355X: 91 tests in 6.7 s, CPU references included (tests/test_gpu_arsample.py, unchanged since the
parent commit: 19 tests in 3.8 s)."""
import pytest
import torch

import arsample_restatement as R
import maf_restatement as MR
from domain_helpers import counts, float64, launched
from torch_nf_amd import _lib as L_, arsample_ops

pytestmark = pytest.mark.gpu

lib = L_.lib
BWD_FAMILIES = (L_.DIAG_MAF_BWD_MFMA, L_.DIAG_MAF_BWD_GENERIC)
PER_CONTEXT = MR.BWD_ROWS[1]  # (3, 3, 147)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def sweep(tnf, oracle):
    """The cases and their bars: each section is built once, on the CPU, by the first test that needs it."""
    return R.Sweep(tnf, oracle)


_WORST = {}  # group -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error, %s: %.3f of the bar" % (name, frac))


def under(sweep, group, L, got, want, what):
    e, bar = MR.gerr(got, want), sweep.bar(group, L)
    _WORST[group] = max(e / bar, _WORST.get(group, 0.0))
    print("%s, %s L=%d: %.3e, %.3f of the bar" % (what, group, L, e, e / bar))
    assert bool(torch.isfinite(got).all()) and e <= bar, "%s, %s: error %.3e exceeds %.3e" % (what, group, e, bar)


def one_launch(before):
    """Since `before` = (arsample count, diag counters): exactly one call reached the kernel and no diag family moved."""
    return (arsample_ops.arsample_launch_count() - before[0], launched(before[1])) == (1, {})


def mark():
    return arsample_ops.arsample_launch_count(), counts()


def run_maf(c, x=None, params=None, g_x="own", g_ld="own", want_omega=True):
    """One tnf_maf_sample_bwd_f32 call on the case's inputs (or the given device tensors) -> (g_omega, g_params) on the CPU."""
    x = c.x.cuda() if x is None else x
    params = c.params.cuda() if params is None else params
    g_x = c.g_x.cuda() if isinstance(g_x, str) else g_x
    g_ld = c.g_ld.cuda() if isinstance(g_ld, str) else g_ld
    before = mark()
    go, gp = arsample_ops.maf_sample_bwd_raw(x, params, c.layer._masks_for(torch.float32), g_x, g_ld, *c.shape, want_omega)
    assert one_launch(before), (c.shape, c.rows)
    assert gp.shape == c.params.shape and (go is None) == (not want_omega)
    return (None if go is None else go.cpu()), gp.cpu()


def what_of(c):
    return "%s (%d, %d, %d)" % (MR.case_id(*c.shape), *c.rows)


def private_rows(c):
    """Is the call bit-reproducible as include/tnf_arsample.h promises: per-context rows and four private copies?"""
    return c.rows[1] > 1 and MR.nacc(*c.shape) == 4


# ---- a. the bijector entry over every cell ----------------------------------------------------------------------------------
def _id(s):
    return "%s-nacc%d" % (MR.case_id(*s), MR.nacc(*s))


@pytest.mark.parametrize("D,L,U", R.maf_shapes(), ids=[_id(s) for s in R.maf_shapes()])
def test_maf_cell(tnf, sweep, D, L, U):
    """One shared row in one workgroup (1, 1, 37), per-context rows with one workgroup walking 10 tiles (3, 3, 147), three
    contexts flushing into one row by atomics (3, 1, 37)."""
    sweep.need("maf")
    assert lib.tnf_maf_sample_bwd_supported(D, L, U) == 1
    for rows in MR.BWD_ROWS:
        c = sweep.maf[((D, L, U), rows)]
        go, gp = run_maf(c)
        under(sweep, "maf g_omega", L, go, c.f64[0], what_of(c))
        under(sweep, "maf g_params", L, gp, c.f64[1], what_of(c))
        idx = c.masked_columns()
        assert idx and float(gp[:, idx].abs().max()) == 0.0, "%s: a masked weight has a gradient" % what_of(c)
        if private_rows(c):
            again = run_maf(c)
            assert torch.equal(go, again[0]) and torch.equal(gp, again[1]), "%s: not bit-reproducible" % what_of(c)


# ---- b. argument paths ---------------------------------------------------------------------------------------------------------
def _f64(c, g_x=True, g_ld=True):
    """The float64 restatement with one cotangent absent."""
    z = torch.zeros((), dtype=torch.float64)
    with float64(), torch.no_grad():
        return R.maf_sample_bwd(c.x.double(), c.params.double(), c.Ms, c.g_x.double() if g_x else z * c.g_x.double(),
                                c.g_ld.double() if g_ld else z * c.g_ld.double(), *c.shape)[:2]


@pytest.mark.parametrize("D,L,U", R.ARG_CELLS, ids=[_id(s) for s in R.ARG_CELLS])
def test_optional_arguments(tnf, sweep, D, L, U):
    """g_x == NULL, g_ld == NULL (the NULL branches of the load stage: autograd's zero cotangents never take them),
    g_omega == NULL, and a parameter row stride beyond the row with NaN in the gap."""
    sweep.need("maf")
    c = sweep.maf[((D, L, U), PER_CONTEXT)]
    exact, what = private_rows(c), what_of(c)
    assert exact == (MR.nacc(D, L, U) == 4)

    def same(a, b, tag):
        if exact:
            assert all(torch.equal(p, q) for p, q in zip(a, b) if p is not None and q is not None), "%s: %s" % (what, tag)

    base = run_maf(c)
    for tag, kw, want in (("g_x", dict(g_x=None), _f64(c, g_x=False)), ("g_ld", dict(g_ld=None), _f64(c, g_ld=False))):
        got = run_maf(c, **kw)
        zeros = run_maf(c, **{tag: torch.zeros_like(getattr(c, tag)).cuda()})
        same(got, zeros, tag + " = None against zeros")
        for out in (got, zeros):
            under(sweep, "maf g_omega", L, out[0], want[0], "%s %s absent" % (what, tag))
            under(sweep, "maf g_params", L, out[1], want[1], "%s %s absent" % (what, tag))
    got = run_maf(c, want_omega=False)
    same((got[1],), (base[1],), "want_omega = False")
    under(sweep, "maf g_params", L, got[1], c.f64[1], what + " without g_omega")
    wide = torch.full((c.rows[1], c.P + 5), float("nan"), device="cuda")
    wide[:, :c.P] = c.params.cuda()
    view = wide[:, :c.P]
    assert view.stride() == (c.P + 5, 1) and bool(torch.isnan(wide[:, c.P:]).all())
    got = run_maf(c, params=view)
    same(got, base, "pstride > P")
    under(sweep, "maf g_omega", L, got[0], c.f64[0], what + " pstride > P")
    under(sweep, "maf g_params", L, got[1], c.f64[1], what + " pstride > P")


@pytest.mark.parametrize("D,L,U", R.ARG_CELLS, ids=[_id(s) for s in R.ARG_CELLS])
def test_row_edges_and_many_contexts(tnf, sweep, D, L, U):
    """N = 1, 15, 16, 17 (padded rows of a tile must add nothing) and 130 contexts, per-context rows and one shared row."""
    sweep.need("args")
    for rows in [(1, 1, N) for N in R.EDGE_NS] + R.MANY_ROWS:
        c = sweep.args[((D, L, U), rows)]
        go, gp = run_maf(c)
        under(sweep, R.arg_group(rows) + " g_omega", L, go, c.f64[0], what_of(c))
        under(sweep, R.arg_group(rows) + " g_params", L, gp, c.f64[1], what_of(c))
        assert float(gp[:, c.masked_columns()].abs().max()) == 0.0


def test_prefilled_g_params(tnf, sweep):
    """include/tnf_arsample.h: with per-context rows the MAF block is WRITTEN (a prefill of 1.0 leaves no trace, bit for
    bit) and the Affine slice of the stack entry is ADDED to (1 + the gradient); callers zero g_params in every case.
    One ctypes call per entry and prefill, private-copy cell."""
    sweep.need("maf").need("flow")
    s = R.ALIGN_CELL
    c = sweep.maf[(s, PER_CONTEXT)]
    M, Mp, N = c.rows
    x, p, gx, gl = c.x.cuda(), c.params.cuda(), c.g_x.cuda(), c.g_ld.cuda()
    mk = c.layer._masks_for(torch.float32)
    out = {}
    for fill in (0.0, 1.0):
        gp = torch.full((Mp, c.P), fill, device="cuda")
        L_.check(lib.tnf_maf_sample_bwd_f32(x.data_ptr(), p.data_ptr(), mk.data_ptr(), gx.data_ptr(), gl.data_ptr(), None,
                                            gp.data_ptr(), M, Mp, N, *s, c.P, c.P, L_.stream_ptr()))
        out[fill] = gp.cpu()
    assert torch.equal(out[0.0], out[1.0])
    under(sweep, "maf g_params", s[1], out[1.0], c.f64[1], what_of(c) + " prefilled")
    s = next(t for t in R.flow_shapes() if MR.nacc(*t) == 4)
    f = sweep.flow[(s, R.FLOW_ROWS[0])]
    M, Mp, N = f.rows
    P = f.params.shape[1]
    z, p, gz, gs = f.z.cuda(), f.params.cuda(), f.g_z.cuda(), f.g_sld.cuda()
    mk, mean, alpha = f.nf.bijectors[0]._masks_for(torch.float32), f.stat[0].cuda(), f.stat[1].cuda()
    nbytes = L_.check(lib.tnf_ar_flow_sample_bwd_workspace_bytes(Mp, s[0]))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for fill in (0.0, 1.0):
        gp = torch.full((Mp, P), fill, device="cuda")
        L_.check(lib.tnf_ar_flow_sample_bwd_f32(z.data_ptr(), p.data_ptr(), mk.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                                gz.data_ptr(), gs.data_ptr(), gp.data_ptr(), M, Mp, N, *s, P, P, ws.data_ptr(),
                                                nbytes, L_.stream_ptr()))
        out[fill] = gp.cpu()
    assert torch.equal(f.split(out[0.0])[0], f.split(out[1.0])[0])
    torch.testing.assert_close(f.split(out[1.0])[1], 1.0 + f.split(out[0.0])[1], rtol=2e-7, atol=2e-7)
    under(sweep, "flow g_maf", s[1], f.split(out[0.0])[0], f.split(f.f64["both"])[0], "flow %s zero-filled" % MR.case_id(*s))
    under(sweep, "flow g_affine", s[1], f.split(out[0.0])[1], f.split(f.f64["both"])[1], "flow %s zero-filled" % MR.case_id(*s))


def test_unaligned_rows_take_the_scalar_loads(tnf, sweep):
    """x and g_x as contiguous views 4 bytes past a 16-byte boundary (a narrowed view out of the backward of torch.cat is
    one): launch_maf_sample_bwd takes the VEC instantiation only for 16-byte aligned x, g_x and g_omega, so this call runs
    the non-VEC kernel at D = 16 -- one launch, the aligned call's result within the bar.  By construction only: nothing
    here can tell which instantiation ran, and the hardware tolerates dword-aligned float4 accesses, so the test would
    pass without the launcher's predicate; it is no proof of the dispatch.  g_omega is allocated by the wrapper and is
    always aligned, so its part of the predicate is not exercised."""
    sweep.need("maf")
    s = R.ALIGN_CELL
    c = sweep.maf[(s, PER_CONTEXT)]
    assert s[0] % 4 == 0 and private_rows(c)

    def shifted(t):
        buf = torch.empty(t.numel() + 4, device="cuda")
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    aligned = run_maf(c)
    got = run_maf(c, x=shifted(c.x), g_x=shifted(c.g_x))
    for i, part in enumerate(("g_omega", "g_params")):
        under(sweep, "maf " + part, s[1], got[i], c.f64[i], what_of(c) + " unaligned")
        assert MR.gerr(got[i], aligned[i]) <= sweep.bar("maf " + part, s[1])


# ---- c. the stack entry -------------------------------------------------------------------------------------------------------
def run_flow(f, g_z, g_sld):
    mk = f.nf.bijectors[0]._masks_for(torch.float32)
    p = f.params.cuda()
    before = mark()
    gp = arsample_ops.ar_flow_sample_bwd_raw(f.z.cuda(), p, p.shape[1], mk, f.stat[0].cuda(), f.stat[1].cuda(),
                                             None if g_z is None else g_z.cuda(), None if g_sld is None else g_sld.cuda(),
                                             *f.shape, tuple(p.shape))
    assert one_launch(before), (f.shape, f.rows)
    return gp.cpu()


@pytest.mark.parametrize("D,L,U", R.flow_shapes(), ids=[_id(s) for s in R.flow_shapes()])
def test_flow_cell(tnf, sweep, D, L, U):
    """The AR-stack mode: the fold in the load stage, its three sums, the finalize kernel; a None cotangent is a NULL."""
    sweep.need("flow")
    for rows in R.FLOW_ROWS:
        f = sweep.flow[((D, L, U), rows)]
        for name, g_z, g_sld in f.cotangents(none=True):
            what = "flow %s (%d, %d, %d) %s" % (MR.case_id(D, L, U), *rows, name)
            gp = run_flow(f, g_z, g_sld)
            under(sweep, "flow g_maf", L, f.split(gp)[0], f.split(f.f64[name])[0], what)
            under(sweep, "flow g_affine", L, f.split(gp)[1], f.split(f.f64[name])[1], what)


# ---- d. long rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,U", MR.LONG_CELLS, ids=[_id(s) for s in MR.LONG_CELLS])
def test_long_row(tnf, sweep, D, L, U):
    """One shared row of 32,789 samples: 2,050 tiles on the 512-workgroup cap, a second tile per wave, every workgroup
    flushing through atomics; one shared-copy and one private-copy cell."""
    sweep.need("long")
    N = MR.LONG_N
    assert MR.bwd_bx(N, 1) == 512 and MR.tiles_per_wave(N, 512) == 2
    assert MR.nacc(D, L, U) == (1 if (D, L, U) == MR.LONG_CELLS[0] else 4)
    c = sweep.long[(D, L, U)]
    go, gp = run_maf(c)
    under(sweep, "long g_omega", L, go, c.f64[0], what_of(c))
    under(sweep, "long g_params", L, gp, c.f64[1], what_of(c))
    assert float(gp[:, c.masked_columns()].abs().max()) == 0.0


# ---- e. NormFlow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,U", R.nf_shapes(), ids=[_id(s) for s in R.nf_shapes()])
def test_normflow_route(tnf, sweep, D, L, U):
    """The flow as a user trains it: the one-kernel inference forward in front, tnf_ar_flow_sample_bwd_f32 behind."""
    sweep.need("nf")
    f, want = sweep.nf[(D, L, U)]
    nf = f.nf
    nf.bijectors[1].set_last_stats(f.stat[0].cuda(), f.stat[1].cuda())
    omega, wz, wl = f.omega.cuda(), f.g_z.cuda(), f.g_sld.cuda()
    nf.ar_sample_training = True
    try:
        p = f.params.cuda().requires_grad_()
        assert nf._route("forward", omega, p) == ("ar_train_sample", False, False)
        with torch.no_grad():
            z_inf, lq_inf = nf._forward_from(omega, p, freeze_bn=True)
        before = mark()
        z, lq = nf._forward_from(omega, p, freeze_bn=True)
        ((z * wz).sum() + (lq * wl).sum()).backward()
        assert one_launch(before)
    finally:
        nf.ar_sample_training = False
    assert torch.equal(z.detach(), z_inf) and torch.equal(lq.detach(), lq_inf)
    what = "NormFlow %s (%d, %d, %d)" % (MR.case_id(D, L, U), *f.rows)
    gp = p.grad.cpu()
    under(sweep, "nf g_maf", L, f.split(gp)[0], f.split(want)[0], what)
    under(sweep, "nf g_affine", L, f.split(gp)[1], f.split(want)[1], what)


# ---- f. the small-weight regime -----------------------------------------------------------------------------------------------
def test_small_weights(tnf, sweep):
    """Weights 0.05, L = 3: pre-activations near 0, every r near 1/2, and h = 1 - 2 r carries the ABSOLUTE quantisation of
    r (6e-8) whatever the size of h -- the relative error of the weight gradients that h enters grows as the weights
    shrink, without bound.  CAP is a statement about the O(1) regime MR.weight_scale keeps; this group's bar is what the
    restatement gives on these inputs, whichever side of CAP that is."""
    sweep.need("small")
    c = sweep.small
    D, L, U = c.shape
    assert MR.bwd_supported(D, L, U) and float(c.params.abs().max()) < 0.3
    go, gp = run_maf(c)
    under(sweep, "small-weight g_omega", L, go, c.f64[0], what_of(c))
    under(sweep, "small-weight g_params", L, gp, c.f64[1], what_of(c))


# ---- g. refused shapes ----------------------------------------------------------------------------------------------------------
REFUSED = R.refused_shapes() + [(33, 2, 17), (6, 4, 15)]


@pytest.mark.parametrize("D,L,U", REFUSED, ids=[MR.case_id(*s) for s in REFUSED])
def test_refused_shapes_run_the_composition(tnf, oracle, D, L, U):
    """No kernel for the shape: the switch changes nothing, the backward is tnf_maf_inverse_alpha and D + 1 tnf_maf_backward
    launches, and the gradient holds the composition's bound CAP."""
    assert lib.tnf_maf_sample_bwd_supported(D, L, U) == 0
    c = R.SampleCase(tnf, oracle, D, L, U, 2, 2, 20)
    c.layer.fused_sampling_backward = True
    p, om = c.params.cuda().requires_grad_(), c.omega.cuda().requires_grad_()
    before = mark()
    x, ld = c.layer(om, p)
    ((x * c.g_x.cuda()).sum() + (ld * c.g_ld.cuda()).sum()).backward()
    ran = launched(before[1], BWD_FAMILIES)
    assert arsample_ops.arsample_launch_count() == before[0] and sum(ran.values()) == D + 1, ran
    for got, want, part in ((om.grad, c.f64[0], "g_omega"), (p.grad, c.f64[1], "g_params")):
        e = MR.gerr(got.cpu(), want)
        print("refused %s %s: %.3e" % (MR.case_id(D, L, U), part, e))
        assert bool(torch.isfinite(got).all()) and e <= R.CAP
