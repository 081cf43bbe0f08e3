"""The MAF kernels over their own domain against the CPU oracle in float64 -- maf_mfma.hip (both directions and the AR
one-kernel paths around it), maf_bwd_mfma.hip (plain and fused, both accumulator schemes, both flushes), the two-pass
wide backward of coupling_wide_bwd.hip and the shape-generic kernels they fall back to -- in the pattern of
tests/test_gpu_support_domain.py.  Helpers, grid and inputs: tests/maf_restatement.py; the host half, which pins the
noise model and the grid's coverage without a GPU: tests/test_maf_host.py.

Reference: oracle/flow_oracle.py under domain_helpers.float64() on float64 copies of the float32 inputs.  Error:
max |got - want| / max(1, max |want|), the denominator taken over the whole case (every row layout of a case is a slice
of one batch, and the noise behind the bar is measured against the same value); gradients: conftest.grad_err's measure.
Inputs: masks by the package's rule (np.random.seed, then tnf.MAF), weights ~ N(0, 0.4 / sqrt(max(1, U / 16))), z ~ N(0, 1).

Bars.  The matrix-pipe kernels carry every hidden activation as r = 1 / (1 + 2^a), fold -2 c W and the column sums into
operands and accumulator seeds and keep alpha in log2 units; in float32 that is 2 .. 10 x noisier than the oracle's own
float32.  So each case evaluates that formulation restated in float32 torch (MR.folded_maf) on its own inputs, and the
bar of a group (quantity, L) is 4 x the largest such error in the group -- the margin of conftest.grad_err's bars: room for
another summation order and 1-ulp hardware exp2 / rcp, not for a lower precision class.  The shape-generic kernels are
held to 4 x the float32 oracle's own error.  Float64 kernels: rtol = atol = 1e-11.  No bar comes from a kernel's output.

a  MAF.inverse_and_log_det / forward_and_log_det, float32: every (DT, UT) cell at D = 16 (DT - 1) + 1 (2 for DT = 1),
   16 DT - 4, 16 DT; U = 16 (UT - 1) + 1 (5 for UT = 1), 16 UT; L = 1, 2, and L = 3, the largest supported L and every
   refused L at the (16 DT, 16 UT) corner; rows (M_z, M_p, N) = (1,1,1), (1,1,15), (1,1,16), (1,1,17), (3,3,65),
   (3,1,33), (1,3,33); every call again under OPT_FORCE_GENERIC.  The four refused cells (DT, L, UT) = (2,5,4), (3,5,4),
   (4,4,4), (4,5,4): tnf_ar_flow_supported == 0 and the default call equals the forced-generic one bit for bit.  Tile
   walk: (512, 512, 277) and (512, 1, 277) at one shape per DT -- 4 workgroups for 18 tiles, a second, ragged tile.
b  The generic kernels beyond the matrix-pipe domain: D = 65, 100, U = 65, float32 and float64.
c  NormFlow(D, True, "AR", 1, L, U) with frozen statistics on the same cells: log_prob, z0, sum_log_det, the frozen
   forward's z and log_q, each route asserted through NormFlow._route.
d  Backward of inverse_and_log_det: every (DT <= 2, UT, VEC) cell, L = 1, 2, 3, rows (1,1,37), (3,3,147) (one workgroup
   walks 10 tiles), (3,1,37); launch counters in both directions; masked weights exactly zero; the two-pass wide backward
   at D = 36, 64 x every UT x L = 1, 2, row (2,1,37); D > 32 with per-context rows asserted onto the generic kernel.
e  ar_train: every (DT <= 2, UT, L) cell, M_p = M and 1, N = 37, 147, upstream weights 10^U(-3, 0); N = 32,789 with one
   shared row on a fixed-point and on a private-copy cell (2,050 tiles on 512 workgroups: adds = 5, fbits = 15, a second
   tile per wave); with M_p > 1 two runs give a bit-identical MAF block (one workgroup per row, a fixed tile-to-wave
   assignment, private copies or integer adds).  Refused cells run the per-bijector route, asserted.
f  Weights 0.05, L = 3 (D = 16, U = 32): the last hidden r sits near 1/2, where its absolute quantisation of 1.2e-7 is
   1e-5 of h = 1 - 2 r; a group of its own with the bar from the restatement on those inputs.

Noise of each group (quantity, L) -- the folded restatement in float32 against the float64 oracle on the sweep's inputs;
"generic": the oracle's own float32; "unfused": the larger of the two -- as the CPU computes it where the host half was
written (each run recomputes it and prints it with the bar when a section is built).  The bar is 4 x the entry.
  quantity                        L=1      L=2      L=3      L=4      L=5
  generic inverse ld              3.0e-07  5.0e-07  2.6e-07  3.5e-07  4.5e-07
  generic inverse z               8.1e-07  6.4e-07  3.3e-07  3.1e-07  2.3e-07
  generic sampling ld             3.6e-07  4.8e-07  3.0e-07  3.5e-07  4.4e-07
  generic sampling z              9.2e-07  7.0e-07  2.9e-07  2.5e-07  3.4e-07
  inverse ld                      1.1e-06  2.4e-06  1.8e-06  1.6e-06  2.8e-06
  inverse z                       1.1e-06  1.4e-06  1.1e-06  8.0e-07  8.4e-07
  sampling ld                     1.1e-06  2.4e-06  1.3e-06  1.9e-06  2.6e-06
  sampling z                      1.4e-06  1.5e-06  8.2e-07  1.4e-06  9.6e-07
  tile walk inverse ld            -        5.4e-07  -        -        -
  tile walk inverse z             -        4.8e-07  -        -        -
  tile walk sampling ld           -        5.4e-07  -        -        -
  tile walk sampling z            -        5.0e-07  -        -        -
  AR lp                           8.7e-07  1.4e-06  3.6e-07  4.5e-07  6.4e-07
  AR lq                           4.1e-07  1.9e-07  4.5e-08  6.9e-08  1.2e-07
  AR sld                          4.4e-07  1.7e-06  8.6e-07  1.1e-06  2.5e-06
  AR z0                           6.9e-07  8.1e-07  9.2e-07  8.5e-07  9.5e-07
  AR zf                           1.3e-06  7.7e-07  4.6e-07  6.4e-07  9.0e-07
  backward g_params               1.1e-06  3.6e-06  2.1e-06  -        -
  backward g_z                    1.0e-06  1.3e-06  1.2e-06  -        -
  generic backward g_params       7.3e-07  1.2e-06  8.6e-07  -        -
  generic backward g_z            5.6e-07  5.0e-07  5.5e-07  -        -
  small-weight backward g_params  -        -        1.4e-04  -        -
  small-weight backward g_z       -        -        1.0e-07  -        -
  ar_train g_params               1.6e-06  1.4e-06  2.6e-06  -        -
  unfused ar_train g_params       -        1.5e-06  1.7e-06  -        -
Largest error / bar per group on the MI355X (the module prints each case's, and these when it is done): inverse z 0.35,
log-det 0.35; sampling z 0.29, log-det 0.35; tile walk at most 0.21; generic inverse z 0.34, log-det 0.29, sampling z
0.30, log-det 0.29; AR log_prob 0.42, z0 0.42, sum_log_det 0.32, frozen z 0.31, log_q 0.27; backward g_z 0.21, g_params
0.33 (generic 0.36, 0.32); ar_train g_params 0.29, on the 32,789-sample rows 0.17, unfused 0.12; small-weight backward
g_z 0.21, g_params 0.02.  Nothing exceeded its bar; every bit-identity of (e) and every route held."""
import contextlib

import pytest
import torch

import maf_restatement as MR
from conftest import grad_err
from domain_helpers import counts, launched
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
F64_TOL = dict(rtol=1e-11, atol=1e-11)
BWD_FAMILIES = (L_.DIAG_MAF_BWD_MFMA, L_.DIAG_MAF_BWD_GENERIC)
CELLS = [(DT, UT) for DT in MR.DTS for UT in MR.UTS]
CELL_IDS = ["DT%d-UT%d" % c for c in CELLS]


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def sweep(tnf, oracle):
    """The cases and their bars: each section is built once, on the CPU, by the first test that needs it."""
    return MR.Sweep(tnf, oracle)


_WORST = {}  # group -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error, %s: %.3f of the bar" % (name, frac))


def under(sweep, group, L, got, want, what, measure=MR.err, scale=None):
    """The float32 comparison: `measure` against the group's bar; prints and notes error / bar.  `scale`: the case's
    denominator of MR.err -- a layout is a slice of its case and is measured against the case's largest value, as the
    noise behind the bar is."""
    e, bar = (measure(got, want) if scale is None else measure(got, want, scale)), sweep.bar(group, L)
    _WORST[group] = max(e / bar, _WORST.get(group, 0.0))
    print("%s, %s L=%d: %.3f of the bar" % (what, group, L, e / bar))
    assert bool(torch.isfinite(got).all()) and e <= bar, "%s, %s: error %.3e exceeds %.3e" % (what, group, e, bar)


@contextlib.contextmanager
def forced_generic():
    L_.check(lib.tnf_set_option(L_.OPT_FORCE_GENERIC, 1))
    try:
        yield
    finally:
        L_.check(lib.tnf_set_option(L_.OPT_FORCE_GENERIC, 0))


def run_maf(c, inverse, Mz, Mp, N, dtype=torch.float32):
    z, p = c.inputs(Mz, Mp, N)
    fn = c.layer.inverse_and_log_det if inverse else c.layer.forward_and_log_det
    with torch.no_grad():
        out, ld = fn(z.to(dtype).cuda(), p.to(dtype).cuda())
    M = max(Mz, Mp)
    assert out.shape == (M, N, c.D) and ld.shape == (M, N) and out.dtype == ld.dtype == dtype
    return out.cpu(), ld.cpu()


# ---- a. MAF forward and inverse, float32 -----------------------------------------------------------------------------------
def check_forward(sweep, c, rows, prefix="", generic=True):
    D, L, U = c.D, c.L, c.U
    sup = MR.fwd_supported(D, L, U)
    assert bool(lib.tnf_ar_flow_supported(D, L, U)) == sup
    for inverse, name in ((True, "inverse"), (False, "sampling")):
        sz, sl = c.scale(inverse)
        for Mz, Mp, N in rows:
            what = "%s (%d, %d, %d)" % (MR.case_id(D, L, U), Mz, Mp, N)
            want = c.want(inverse, Mz, Mp, N)
            got = run_maf(c, inverse, Mz, Mp, N)
            if sup:
                under(sweep, "%s%s z" % (prefix, name), L, got[0], want[0], what, scale=sz)
                under(sweep, "%s%s ld" % (prefix, name), L, got[1], want[1], what, scale=sl)
            if not generic:
                continue
            with forced_generic():
                gen = run_maf(c, inverse, Mz, Mp, N)
            under(sweep, "generic %s z" % name, L, gen[0], want[0], what, scale=sz)
            under(sweep, "generic %s ld" % name, L, gen[1], want[1], what, scale=sl)
            if not sup:  # no matrix-pipe kernel: the default call IS the generic kernel
                assert torch.equal(got[0], gen[0]) and torch.equal(got[1], gen[1]), what
            elif N >= 33:  # two arithmetics: equal bits on this many values would mean the switch selected nothing
                assert not torch.equal(got[0], gen[0]), what


@pytest.mark.parametrize("DT,UT", CELLS, ids=CELL_IDS)
def test_forward_cell(tnf, sweep, DT, UT):
    sweep.need("forward")
    for s in MR.forward_cell(DT, UT):
        assert MR.tiles(s[0], s[2]) == (DT, UT)
        check_forward(sweep, sweep.fwd[s], MR.ROWS)
    refused = [s for s in MR.forward_cell(DT, UT) if not MR.fwd_supported(*s)]
    assert [(DT, s[1], UT) for s in refused] == [c for c in MR.UNSUPPORTED_FWD if (c[0], c[2]) == (DT, UT)]


@pytest.mark.parametrize("DT", MR.DTS)
def test_forward_tile_walk(tnf, sweep, DT):
    """2048 / 512 = 4 workgroups per context for 18 tiles: 16 waves, two of them walk a second tile, the last one ragged
    (277 = 17 * 16 + 5); per-context and shared parameter rows."""
    sweep.need("walk")
    for Mz, Mp, N in MR.WALK_ROWS:
        assert MR.fwd_bx(N, max(Mz, Mp)) == 4 and MR.tiles_per_wave(N, 4) == 2 and N % 16 != 0
    check_forward(sweep, sweep.walk[DT], MR.WALK_ROWS, prefix="tile walk ", generic=False)


# ---- b. the generic kernels beyond the matrix-pipe domain ---------------------------------------------------------------------
@pytest.mark.parametrize("D,L,U", MR.GENERIC_SHAPES, ids=[MR.case_id(*s) for s in MR.GENERIC_SHAPES])
def test_generic_beyond_the_domain(tnf, sweep, D, L, U):
    sweep.need("forward")
    c = sweep.generic[(D, L, U)]
    assert lib.tnf_ar_flow_supported(D, L, U) == 0
    for inverse, name in ((True, "inverse"), (False, "sampling")):
        sz, sl = c.scale(inverse)
        for Mz, Mp, N in ((3, 3, 65), (3, 1, 33), (1, 3, 33)):
            what = "%s (%d, %d, %d)" % (MR.case_id(D, L, U), Mz, Mp, N)
            want = c.want(inverse, Mz, Mp, N)
            got = run_maf(c, inverse, Mz, Mp, N)
            under(sweep, "generic %s z" % name, L, got[0], want[0], what, scale=sz)
            under(sweep, "generic %s ld" % name, L, got[1], want[1], what, scale=sl)
            got = run_maf(c, inverse, Mz, Mp, N, torch.float64)
            torch.testing.assert_close(got[0], want[0], **F64_TOL)
            torch.testing.assert_close(got[1], want[1], **F64_TOL)


# ---- c. the AR one-kernel paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("DT,UT", CELLS, ids=CELL_IDS)
def test_ar_cell(tnf, sweep, DT, UT):
    """tnf_ar_flow_log_prob_f32 / tnf_ar_flow_forward_f32 without a support layer: the fold of ar_fold_kernel in the
    kernel's `pre` / `post` stage, the base density in its epilogue (tests/test_gpu_support_domain.py sweeps ToInterval)."""
    sweep.need("ar")
    for s in MR.ar_cell(DT, UT):
        c = sweep.ar[s]
        D, L, U = s
        assert MR.tiles(D, U) == (DT, UT) and lib.tnf_ar_flow_supported(D, L, U) == 1
        scale = c.scale()
        for Mz, Mp, N in MR.AR_ROWS:
            what = "AR %s (%d, %d, %d)" % (MR.case_id(*s), Mz, Mp, N)
            r = {k: v[:Mz, :N] for k, v in c.ref(Mp)["f64"].items()}
            z, p = c.z[:Mz, :N].cuda(), c.params[:Mp].cuda()
            with torch.no_grad():
                for op in ("log_prob", "inverse"):
                    assert c.nf._route(op, z, p) == ("ar_fused", False, False)
                assert c.nf._route("forward", z, p, True) == ("ar_fused", False, False)
                lp = c.nf.log_prob(z, p)
                z0, sld = c.nf.inverse_and_log_det(z, p)
                zf, lq = c.nf._forward_from(z.double(), p, freeze_bn=True)
            assert lq.dtype == torch.float64
            for k, got in (("lp", lp), ("z0", z0), ("sld", sld), ("zf", zf), ("lq", lq)):
                under(sweep, "AR " + k, L, got.cpu(), r[k], what, scale=scale[k])


# ---- d. backward of inverse_and_log_det ---------------------------------------------------------------------------------------
def run_backward(g):
    c = g.case
    p, z = g.params.cuda().requires_grad_(), g.z.cuda().requires_grad_()
    before = counts()
    out, ld = c.layer.inverse_and_log_det(z, p)
    ((out * g.wz.cuda()).sum() + (ld * g.wl.cuda()).sum()).backward()
    return z.grad.cpu(), p.grad.cpu(), launched(before, BWD_FAMILIES)


def check_backward(sweep, g, route, group="backward"):
    """The default call on its expected route and the forced-generic call, counters in both directions."""
    c = g.case
    L, what = c.L, "%s (%d, %d, %d)" % (MR.case_id(c.D, c.L, c.U), g.M, g.Mp, g.N)
    family = L_.DIAG_MAF_BWD_GENERIC if route == "generic" else L_.DIAG_MAF_BWD_MFMA
    gz, gp, ran = run_backward(g)
    assert ran == {family: 1}, (what, route, ran)
    name = "generic backward" if route == "generic" else group
    under(sweep, name + " g_z", L, gz, g.f64[0], what, MR.gerr)
    under(sweep, name + " g_params", L, gp, g.f64[1], what, MR.gerr)
    grad_err("MAF sweep, %s backward: d params" % route, gp, g.f64[1])
    idx = g.masked_columns()
    assert idx and float(gp[:, idx].abs().max()) == 0.0, "%s: a masked weight has a gradient" % what
    with forced_generic():
        gz, gp, ran = run_backward(g)
    assert ran == {L_.DIAG_MAF_BWD_GENERIC: 1}, (what, ran)
    under(sweep, "generic backward g_z", L, gz, g.f64[0], what, MR.gerr)
    under(sweep, "generic backward g_params", L, gp, g.f64[1], what, MR.gerr)
    assert float(gp[:, idx].abs().max()) == 0.0


def _bwd_id(s):
    return "%s-%s" % (MR.case_id(*s), "nacc%d" % MR.nacc(*s) if MR.bwd_supported(*s) else "generic")


@pytest.mark.parametrize("D,L,U", MR.backward_cases(), ids=[_bwd_id(s) for s in MR.backward_cases()])
def test_backward(tnf, sweep, D, L, U):
    """maf_bwd_mfma_kernel in plain mode: nacc = 4 private accumulator copies or one shared copy under float atomics (the
    id names which); plain stores for (3, 3, 147), atomics for the shared row.  A cell the kernel refuses (no LDS for one
    accumulator copy) is asserted onto the generic kernel."""
    sweep.need("backward")
    for M, Mp, N in MR.BWD_ROWS:
        assert MR.bwd_bx(N, Mp) == 1 and MR.tiles_per_wave(147, 1) == 3
        check_backward(sweep, sweep.bwd[(D, L, U, M, Mp, N)], MR.backward_route(D, L, U, Mp))


@pytest.mark.parametrize("D,L,U", MR.wide_cases(), ids=[MR.case_id(*s) for s in MR.wide_cases()])
def test_backward_wide(tnf, sweep, D, L, U):
    """D = 33 .. 64 with one shared row: maf_wide_bwd_kernel + wide_gw_kernel (counted with the matrix-pipe family)."""
    sweep.need("backward")
    M, Mp, N = MR.WIDE_ROW
    assert MR.backward_route(D, L, U, Mp) == "wide"
    check_backward(sweep, sweep.bwd[(D, L, U, M, Mp, N)], "wide")


@pytest.mark.parametrize("case", MR.GENERIC_BWD, ids=["%s-Mp%d" % (MR.case_id(*g[:3]), g[4]) for g in MR.GENERIC_BWD])
def test_backward_wide_refuses_per_context_rows(tnf, sweep, case):
    sweep.need("backward")
    assert MR.backward_route(*case[:3], case[4]) == "generic" and MR.backward_route(*case[:3], 1) != "mfma"
    check_backward(sweep, sweep.bwd[case], "generic")


# ---- e. ar_train ----------------------------------------------------------------------------------------------------------
def run_train(t):
    nf = t.ar.nf
    p, z = t.params.clone().cuda().requires_grad_(), t.ar.z.cuda()
    route = nf._route("log_prob", z, p)
    before = counts()
    lp = nf.log_prob(z, p)
    (lp * t.w.cuda()).sum().backward()
    return p.grad.cpu(), lp.detach().cpu(), route, launched(before, BWD_FAMILIES)


def _train_id(s):
    return "%s-%s" % (MR.case_id(*s), MR.train_mode(*s) if MR.train_supported(*s) else "unfused")


@pytest.mark.parametrize("D,L,U", MR.train_cases(), ids=[_train_id(s) for s in MR.train_cases()])
def test_ar_train(tnf, sweep, D, L, U):
    """The fused backward (maf_bwd_mfma_kernel with g_lp): float accumulation in private copies or 32-bit fixed point in
    the shared copy (the id names which), upstream weights over three decades.  The Affine tail leaves through float LDS
    atomics and is held to the bar only; the MAF block of a per-context run is bit-reproducible."""
    sweep.need("train")
    sup = MR.train_supported(D, L, U)
    assert bool(lib.tnf_ar_flow_train_supported(D, L, U)) == sup
    for Mp in (MR.TRAIN_M, 1):
        for N in MR.TRAIN_NS:
            t = sweep.train[(D, L, U, MR.TRAIN_M, Mp, N)]
            what = "ar_train %s (%d, %d, %d)" % (MR.case_id(D, L, U), MR.TRAIN_M, Mp, N)
            gp, lp, route, ran = run_train(t)
            assert float(t.w.max() / t.w.min()) > 100.0
            torch.testing.assert_close(lp.double(), t.lp64, rtol=1e-5, atol=1e-5)  # LOGP_TOL; test_ar_cell holds it to its bar
            if sup:
                assert route == ("ar_train", False, False) and ran == {L_.DIAG_MAF_BWD_MFMA: 1}, (what, route, ran)
                under(sweep, "ar_train g_params", L, gp, t.g64, what, MR.gerr)
                grad_err("MAF sweep, ar_train: d params", gp, t.g64)
                if Mp > 1:
                    again = run_train(t)[0]
                    assert torch.equal(gp[:, :t.ar.p_maf], again[:, :t.ar.p_maf]), "%s: MAF block not reproducible" % what
                    under(sweep, "ar_train g_params", L, again, t.g64, what, MR.gerr)
            else:  # no fused backward for the cell: the per-bijector composition, its MAF backward on the route (d) names
                fam = L_.DIAG_MAF_BWD_GENERIC if MR.backward_route(D, L, U, Mp) == "generic" else L_.DIAG_MAF_BWD_MFMA
                assert route == ("bijectors", False, False) and ran == {fam: 1}, (what, route, ran)
                under(sweep, "unfused ar_train g_params", L, gp, t.g64, what, MR.gerr)


@pytest.mark.parametrize("D,L,U", MR.LONG_CELLS, ids=[_train_id(s) for s in MR.LONG_CELLS])
def test_ar_train_long_row(tnf, sweep, D, L, U):
    """One shared row of 32,789 samples: 2,050 tiles on the 512-workgroup cap, so waves walk a second tile, every
    workgroup flushes by atomics and -- on the fixed-point cell -- 5 terms per accumulator leave 15 fraction bits."""
    sweep.need("train")
    N = MR.LONG_N
    assert MR.bwd_bx(N, 1) == 512 and MR.adds_fbits(N, 1) == (5, 15) and MR.tiles_per_wave(N, 512) == 2
    assert MR.train_supported(D, L, U) and MR.train_mode(D, L, U) == ("fixed" if (D, L, U) == MR.LONG_CELLS[0] else "private")
    t = sweep.train[(D, L, U, 1, 1, N)]
    gp, lp, route, ran = run_train(t)
    assert route == ("ar_train", False, False) and ran == {L_.DIAG_MAF_BWD_MFMA: 1}, (route, ran)
    torch.testing.assert_close(lp.double(), t.lp64, rtol=1e-5, atol=1e-5)
    under(sweep, "ar_train g_params", L, gp, t.g64, "ar_train %s (1, 1, %d)" % (MR.case_id(D, L, U), N), MR.gerr)


# ---- f. the small-weight regime -----------------------------------------------------------------------------------------------
def test_backward_small_weights(tnf, sweep):
    """Weights 0.05, L = 3: pre-activations near 0, every r near 1/2.  h = 1 - 2 r then carries the ABSOLUTE quantisation
    of r (1.2e-7), 1e-5 of an h of 0.01 and hence of the output layer's weight gradient.  Measured and bounded by the
    restatement on these inputs -- a bar two decades above the O(1) regime's, which therefore stays a group of its own."""
    sweep.need("backward")
    g = sweep.small
    D, L, U = MR.SMALL_WEIGHT[:3]
    assert MR.backward_route(D, L, U, 1) == "mfma" and float(g.params.abs().max()) < 0.3
    check_backward(sweep, g, "mfma", group="small-weight backward")
