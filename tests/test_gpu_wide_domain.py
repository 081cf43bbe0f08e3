"""The wide RealNVP kernels over their own domain against the CPU oracle in float64 -- coupling_wide.hip (both directions,
bijector-level calls and the wide per-layer chains of both flow entries), the RealNVP half of coupling_wide_bwd.hip (pass 1,
pass 2 and the ordered reduction) and the shape-generic kernels they fall back to -- in the pattern of
tests/test_gpu_maf_domain.py.  Helpers, grid and inputs: tests/wide_restatement.py; the host half, which pins the noise
model and the grid's coverage without a GPU: tests/test_wide_host.py.

Reference: oracle/flow_oracle.py under domain_helpers.float64() on float64 copies of the float32 inputs.  Error:
max |got - want| / max(1, max |want|), the denominator taken over the whole case (every row layout of a case is a slice
of one batch, and the noise behind the bar is measured against the same value); gradients: conftest.grad_err's measure.
Inputs: weights and biases ~ N(0, 0.4 / sqrt(max(1, U / 16))), z ~ N(0, 1), the first seed whose float64 reference stays
below 1e3; every reference is asserted finite.

Bars.  The matrix-pipe kernels carry every hidden activation as r = 1 / (1 + 2^a), fold -2 c W and the column sums into
operands and accumulator seeds and keep s in log2 units; in float32 that is up to 3 x noisier than the oracle's own float32.
So each case evaluates that formulation restated in float32 torch (WR.folded_coupling, WR.folded_flow_*) on its own inputs,
and the bar of a group (quantity, L) is 4 x the largest such error in the group -- the margin of conftest.grad_err's bars:
room for another summation order and 1-ulp hardware exp2 / rcp, not for a lower precision class.  Cases on the shape-generic
kernels are held to 4 x the float32 oracle's own error.  Float64 calls: rtol = atol = 1e-11.  No bar comes from a kernel's
output.  Every case names its route in its id and asserts it through the launch counters in both directions: the family
meant moved by the expected count, no other family moved (tnf_coupling's generic kernel has no counter: nothing moves).

a  RealNVP.forward_and_log_det / inverse_and_log_det (U = 5 through ops.coupling, the call they pass through to: the class
   raises num_units to 15), float32, every (HT, UT) cell: D = 32 (HT - 1) + 8, 32 HT - 8, 32 HT; U = 16 (UT - 1) + 1 (5 for
   UT = 1), 16 UT; L = 1, 2, and L = 3, the largest supported L and every refused L at the (32 HT, 16 UT) corner; the
   shapes of the narrow domain run L = 4, 5 instead and (32, 2, 16) is kept, asserted onto coupling_mfma; both transformed
   halves; rows (M_z, M_p, N) = (1,1,16), (1,1,17), (1,1,31), (3,3,65), (3,1,33), (1,3,33); (1,1,15) and (1,1,1) asserted
   onto the generic kernel; every call again under OPT_FORCE_GENERIC; a refused L equals the forced-generic call bit for
   bit.  Tile walk: (512, 512, 129) and (512, 1, 129) at one shape per HT -- 2 workgroups for 9 tiles, a second, ragged
   tile.  One float64 call and one call whose z is offset by 4 bytes per direction: the generic route.
b  tnf_coupling called raw at (72, 2, 33): TNF_LD_ADD and TNF_LD_SUB onto a pre-filled log-det, a parameter row stride 7
   floats longer than the row with NaNs behind it; the wide kernel, the forced-generic call, the oracle.
c  NormFlow at wide shapes with frozen statistics: one padded cell per HT x UT = 2, 4 x S = 1, 3, plus (64, 2, 4, 15) and
   (128, 1, 2, 32); M_p = 1 and M_p = M = 3, N = 33; log_prob, z0, sum_log_det, the frozen forward's z and log_q; route
   "fused" through NormFlow._route and DIAG_COUPLING_WIDE == 2 S per call, under FUSE_LAYER and FUSE_AUTO.
d  Backward of both directions: every (HT, UT) cell at D = 32 HT - 8 and the first U of the tile, L = 1, 2 and 3; rows
   (1,1,37), (3,1,37), (1,1,1); DIAG_BWD_WIDE == 1 per call; against autograd over the float64 oracle and against the
   forced-generic call; asserted onto the generic counter: the LDS-refused (HT, UT, L) = (3,4,2), (4,4,2), L = 3 at
   UT = 3, 4, L = 4, and every cell's (3,3,37).  Slicing at (8, 2, 5): N = 2,049 (129 tiles: 63 empty slices and a ragged
   one), 2,065 (130 tiles, a one-row last tile), 32,789 (2,050 tiles on 512 workgroups); two runs bit-identical.
e  NormFlow(D, "coupling", S = 2, L = 2, U = 20).log_prob(...).sum().backward() at D = 24 and 72, one shared row, N = 37:
   the per-bijector composition, DIAG_BWD_WIDE == 2 S, against autograd over oracle.flow_log_prob in float64.

The flow-level inputs (c, e): statistics as domain_helpers._cde draws them, z = omega ~ N(0, 1), the first of 12 seeds
whose float64 z0 and frozen z stay below 1e3 in both parameter layouts.  At S = 3 no seed does but for one cell -- the
growth is a per-sample product of S factors e^{+-s} per feature, which no per-feature statistic offsets -- and there the
RealNVP weights are the law's divided by sqrt(S) (tests/wide_restatement.py, FlowCase): the bars stay those of an S = 1 flow.

Noise of each group -- the folded restatement in float32 against the float64 oracle on the sweep's inputs; "generic": the
oracle's own float32; "unfused": the larger of the two.  Each run recomputes it and prints it with the bar when a section
is built; the figures differ in the last digit between CPUs.  The bar is 4 x the entry.
  quantity                        L=1      L=2      L=3      L=4      L=5
  generic inverse ld              4.0e-07  4.4e-07  3.6e-07  4.0e-07  5.5e-07
  generic inverse z               1.4e-06  1.6e-06  9.3e-07  1.0e-06  1.2e-06
  generic sampling ld             4.0e-07  4.4e-07  3.6e-07  4.0e-07  5.5e-07
  generic sampling z              1.5e-06  9.8e-07  1.1e-06  1.3e-06  1.3e-06
  inverse ld                      5.5e-07  1.1e-06  8.4e-07  9.7e-07  1.3e-06
  inverse z                       2.0e-06  2.2e-06  2.1e-06  1.8e-06  2.5e-06
  sampling ld                     5.5e-07  1.1e-06  8.4e-07  9.7e-07  1.3e-06
  sampling z                      2.3e-06  1.9e-06  1.6e-06  1.4e-06  2.8e-06
  tile walk inverse / sampling    -        5.1e-07 (z and ld)
  flow S1 lp / z0 / sld           -        2.1e-06 / 3.2e-06 / 2.3e-06
  flow S1 zf / lq                 -        2.6e-06 / 3.4e-07
  flow S2 lp / z0 / sld           -        -        -        1.5e-05 / 9.2e-06 / 1.3e-05
  flow S2 zf / lq                 -        -        -        2.7e-06 / 2.9e-06
  flow S3 lp / z0 / sld           -        2.3e-06 / 4.5e-06 / 8.2e-06
  flow S3 zf / lq                 -        7.9e-06 / 2.8e-06
  backward g_params               1.3e-06  1.4e-06  1.2e-06  -        -
  backward g_z                    1.4e-06  1.3e-06  1.3e-06  -        -
  generic backward g_params       1.4e-06  9.5e-07  8.2e-07  6.2e-07  -
  generic backward g_z            1.1e-06  1.1e-06  7.6e-07  5.5e-07  -
  sliced backward g_params / g_z  -        1.4e-06 / 3.3e-07
  unfused flow backward g_params  -        2.7e-04
Largest error / bar per group on the MI355X (the module prints each case's, and these when it is done; 522 cases in 17 s):
inverse z 0.26, log-det 0.26; sampling z 0.28, log-det 0.26; tile walk at most 0.26; generic inverse z 0.31, log-det 0.35,
sampling z 0.30, log-det 0.35; flows at S = 1: log_prob 0.34, z0 0.19, sum_log_det 0.18, frozen z 0.32, log_q 0.20; S = 2
(L = 4): 0.08, 0.70, 0.74, 0.24, 0.14; S = 3: 0.26, 0.25, 0.13, 0.11, 0.35; backward g_z 0.33, g_params 0.30 (generic 0.27,
0.22); sliced backward g_z 0.18, g_params 0.07; flow backward g_params 0.10.  Nothing exceeded its bar; every route, every
bit-identity and every counter held.  The counters bite: a scratch build whose tnf_coupling sends N < 32 to the generic
kernel fails test_forward on `{} == {DIAG_COUPLING_WIDE: 1}` while tests/test_gpu_parity.py, test_gpu_grad.py and
test_gpu_tight_workspace.py still pass."""
import contextlib

import pytest
import torch

import wide_restatement as WR
from conftest import grad_err
from domain_helpers import counts, launched
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
F64_TOL = dict(rtol=1e-11, atol=1e-11)
BWD_FAMILIES = (L_.DIAG_BWD_WIDE, L_.DIAG_BWD_GENERIC, L_.DIAG_BWD_LAYER_FP32, L_.DIAG_BWD_LAYER_F16, L_.DIAG_BWD_FLOW_REV)
FWD_FAMILY = {"wide": {L_.DIAG_COUPLING_WIDE: 1}, "narrow": {L_.DIAG_COUPLING_MFMA: 1}, "generic": {}}
FORWARD_SHAPES = [s for HT, UT in WR.CELLS for s in WR.forward_cell(HT, UT)] + [WR.NARROW_KEPT]
DIRECTIONS = [(inverse, upper) for inverse in (True, False) for upper in (True, False)]


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@pytest.fixture(scope="module")
def sweep(tnf, oracle):
    """The cases and their bars: each section is built once, on the CPU, by the first test that needs it."""
    return WR.Sweep(tnf, oracle)


_WORST = {}  # group -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error, %s: %.3f of the bar" % (name, frac))


def under(sweep, group, L, got, want, what, measure=WR.err, scale=None):
    """The float32 comparison: `measure` against the group's bar; prints and notes error / bar.  `scale`: the case's
    denominator of WR.err -- a layout is a slice of its case and is measured against the case's largest value, as the
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


def on_gpu(c):
    """The case's rows on the device, copied once."""
    if not hasattr(c, "dev"):
        c.dev = (c.z.cuda(), c.params.cuda())
    return c.dev


def run_layer(tnf, c, inverse, upper, Mz, Mp, N, dtype=torch.float32, z=None):
    """One call of the bijector -> (z_out, log_det, {family: launches})."""
    zd, pd = on_gpu(c)
    z = zd[:Mz, :N].to(dtype) if z is None else z
    if c.U >= 15:
        layer = tnf.RealNVP(c.D, c.L, c.U, transform_upper=upper)
        assert (layer.num_layers, layer.num_units) == (c.L, c.U)
        fn = layer.inverse_and_log_det if inverse else layer.forward_and_log_det
    else:  # the class raises num_units to 15: the call it passes through to
        def fn(z_, p_):
            return tnf.ops.coupling(z_, p_, c.D, c.L, c.U, upper, inverse)
    with torch.no_grad():
        before = counts()
        out, ld = fn(z, pd[:Mp].to(dtype))
        ran = launched(before)
    M = max(Mz, Mp)
    assert out.shape == (M, N, c.D) and ld.shape == (M, N) and out.dtype == ld.dtype == dtype
    return out.cpu(), ld.cpu(), ran


# ---- a. one layer, both directions, float32 --------------------------------------------------------------------------------
def check_forward(tnf, sweep, c, rows, prefix="", generic=True, directions=DIRECTIONS):
    D, L, U = c.D, c.L, c.U
    assert bool(lib.tnf_has_fast_path(D, L, U)) == (WR.wide_supported(D, L, U) or WR.mfma_supported(D, L, U))
    for inverse, upper in directions:
        name = "inverse" if inverse else "sampling"
        sz, sl = c.scale(inverse, upper)
        for Mz, Mp, N in rows:
            route = WR.forward_route(D, L, U, N, M=max(Mz, Mp))
            what = "%s %s (%d, %d, %d) %s" % (WR.case_id(D, L, U), "upper" if upper else "lower", Mz, Mp, N, route)
            want = c.want(inverse, upper, Mz, Mp, N)
            z, ld, ran = run_layer(tnf, c, inverse, upper, Mz, Mp, N)
            assert ran == FWD_FAMILY[route], (what, ran)
            group = "generic " + name if route == "generic" else prefix + name
            under(sweep, group + " z", L, z, want[0], what, scale=sz)
            under(sweep, group + " ld", L, ld, want[1], what, scale=sl)
            if not generic:
                continue
            with forced_generic():
                gz, gld, ran = run_layer(tnf, c, inverse, upper, Mz, Mp, N)
            assert ran == {}, (what, ran)
            under(sweep, "generic %s z" % name, L, gz, want[0], what, scale=sz)
            under(sweep, "generic %s ld" % name, L, gld, want[1], what, scale=sl)
            if route == "generic":  # no matrix-pipe kernel for the call: the default call IS the generic kernel
                assert torch.equal(z, gz) and torch.equal(ld, gld), what
            elif N >= 33:  # two arithmetics: equal bits on this many values would mean the switch selected nothing
                assert not torch.equal(z, gz), what


@pytest.mark.parametrize("inverse", [True, False], ids=["INV1", "INV0"])
@pytest.mark.parametrize("D,L,U", FORWARD_SHAPES, ids=[WR.fwd_id(*s) for s in FORWARD_SHAPES])
def test_forward(tnf, sweep, D, L, U, inverse):
    """coupling_wide_kernel<HT, UT, INV> (the id names the cell, the family and the direction), both halves on every
    shape; N < 16 and every refused L on the generic kernel."""
    sweep.need("forward")
    check_forward(tnf, sweep, sweep.fwd[(D, L, U)], WR.ROWS + WR.GENERIC_ROWS,
                  directions=[d for d in DIRECTIONS if d[0] == inverse])


@pytest.mark.parametrize("HT", WR.HTS, ids=["%s-HT%d-wide" % (WR.case_id(*WR.walk_shape(HT)), HT) for HT in WR.HTS])
def test_forward_tile_walk(tnf, sweep, HT):
    """1024 / 512 = 2 workgroups per context for 9 tiles: 8 waves, one of them walks a second tile, which is ragged
    (129 = 8 * 16 + 1); per-context and shared parameter rows."""
    sweep.need("walk")
    for Mz, Mp, N in WR.WALK_ROWS:
        assert WR.fwd_bx(N, max(Mz, Mp)) == 2 and WR.tiles_per_wave(N, 2) == 2 and N % 16 != 0
    check_forward(tnf, sweep, sweep.walk[HT], WR.WALK_ROWS, prefix="tile walk ", generic=False)


@pytest.mark.parametrize("inverse", [True, False], ids=["inverse-generic", "sampling-generic"])
def test_float64_and_unaligned_take_the_generic_kernel(tnf, sweep, inverse):
    """A float64 call and a float32 call whose z starts 4 bytes past a 16-byte boundary: neither may reach the float4
    loads of the wide kernel."""
    sweep.need("forward")
    c = sweep.fwd[WR.MISC_CELL]
    D, L, U = WR.MISC_CELL
    Mz, Mp, N = 3, 3, 65
    assert WR.forward_route(D, L, U, N) == "wide" and WR.forward_route(D, L, U, N, torch.float64) == "generic"
    assert WR.forward_route(D, L, U, N, aligned=False) == "generic"
    want = c.want(inverse, True, Mz, Mp, N)
    z, ld, ran = run_layer(tnf, c, inverse, True, Mz, Mp, N, torch.float64)
    assert ran == {}, ran
    torch.testing.assert_close(z, want[0], **F64_TOL)
    torch.testing.assert_close(ld, want[1], **F64_TOL)
    buf = torch.empty(Mz * N * D + 1, device="cuda")
    off = buf[1:].view(Mz, N, D)
    off.copy_(on_gpu(c)[0][:Mz, :N])
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    z, ld, ran = run_layer(tnf, c, inverse, True, Mz, Mp, N, z=off)
    assert ran == {}, ran
    with forced_generic():
        gz, gld, _ = run_layer(tnf, c, inverse, True, Mz, Mp, N)
    assert torch.equal(z, gz) and torch.equal(ld, gld)
    sz, sl = c.scale(inverse, True)
    name = "generic %s" % ("inverse" if inverse else "sampling")
    under(sweep, name + " z", L, z, want[0], "unaligned z", scale=sz)
    under(sweep, name + " ld", L, ld, want[1], "unaligned z", scale=sl)


# ---- b. tnf_coupling called raw ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [True, False], ids=["inverse-wide", "sampling-wide"])
def test_raw_log_det_modes_and_row_stride(tnf, sweep, inverse):
    sweep.need("forward")
    D, L, U = WR.RAW_CELL
    c = sweep.fwd[WR.RAW_CELL]
    upper, (Mz, Mp, N), pad = not inverse, (3, 3, 65), 7
    assert WR.forward_route(D, L, U, N) == "wide" and WR.tiles(D, U) == (3, 3) and D // 2 % 16 and U % 16
    zd, pd = on_gpu(c)
    rows = torch.full((Mp, c.P + pad), float("nan"), device="cuda")
    rows[:, :c.P] = pd
    g = torch.Generator().manual_seed(11)
    ld0 = torch.randn(Mz, N, generator=g)
    want = c.want(inverse, upper, Mz, Mp, N)
    sz, sl = c.scale(inverse, upper)
    name = "inverse" if inverse else "sampling"
    for mode, sign in ((L_.LD_ADD, 1.0), (L_.LD_SUB, -1.0)):
        want_ld = ld0.double() + sign * want[1]
        res = []
        for generic in (False, True):
            out, ld = torch.empty(Mz, N, D, device="cuda"), ld0.cuda()
            with forced_generic() if generic else contextlib.nullcontext():
                before = counts()
                L_.check(lib.tnf_coupling(L_.F32, zd.data_ptr(), rows.data_ptr(), out.data_ptr(), ld.data_ptr(), Mz, Mp, N, D, L, U,
                                          int(upper), int(inverse), c.P + pad, mode, L_.stream_ptr()))
                ran = launched(before)
            assert ran == ({} if generic else {L_.DIAG_COUPLING_WIDE: 1}), (mode, generic, ran)
            group, what = ("generic " if generic else "") + name, "raw ld_mode %d, stride P + %d" % (mode, pad)
            under(sweep, group + " z", L, out.cpu(), want[0], what, scale=sz)
            under(sweep, group + " ld", L, ld.cpu(), want_ld, what, scale=sl)
            res.append(out.cpu())
        assert not torch.equal(res[0], res[1])


# ---- c. the wide per-layer chains of the flow entries ---------------------------------------------------------------------------
def _flow_id(s):
    return "D%d-S%d-L%d-U%d-HT%d-UT%d-wide-chain" % (*s, *WR.tiles(s[0], s[3]))


@pytest.mark.parametrize("D,S,L,U", WR.flow_shapes(), ids=[_flow_id(s) for s in WR.flow_shapes()])
def test_flow_chain(tnf, sweep, D, S, L, U):
    """tnf_flow_log_prob_f32 / tnf_flow_forward_f32 on a wide shape: wide_images_kernel, the `pre` / `post` folds of
    flow_fold_kernel and 2 S launches of coupling_wide_kernel, with per-context images (M_p = 3) and one shared one."""
    sweep.need("flow")
    c = sweep.flow[(D, S, L, U)]
    nf, scale = c.nf, c.scale()
    assert lib.tnf_flow_fused_supported(D, S, L, U) == 0 and WR.wide_supported(D, L, U) and not WR.mfma_supported(D, L, U)
    chain = {L_.DIAG_COUPLING_WIDE: 2 * S}
    try:
        for Mz, Mp, N in WR.FLOW_ROWS:
            r = c.ref(Mp)
            zin, om, p = c.z.cuda(), c.z.cuda().double(), c.params[:Mp].cuda()
            for fusion in (L_.FUSE_LAYER, L_.FUSE_AUTO):
                nf.fusion = fusion
                what = "flow D%d S%d L%d U%d (%d, %d, %d) fusion %d" % (D, S, L, U, Mz, Mp, N, fusion)
                with torch.no_grad():
                    for op in ("log_prob", "inverse"):
                        assert nf._route(op, zin, p) == ("fused", False, False), what
                    assert nf._route("forward", om.float(), p, True) == ("fused", False, False), what
                    before = counts()
                    lp = nf.log_prob(zin, p)
                    assert launched(before) == chain, what
                    before = counts()
                    z0, sld = nf.inverse_and_log_det(zin, p)
                    assert launched(before) == chain, what
                    before = counts()
                    zf, lq = nf._forward_from(om, p, freeze_bn=True)
                    assert launched(before) == chain, what
                assert lq.dtype == torch.float64
                for k, got in (("lp", lp), ("z0", z0), ("sld", sld), ("zf", zf), ("lq", lq)):
                    under(sweep, "flow S%d %s" % (S, k), L, got.cpu(), r["f64"][k], what, scale=scale[k])
    finally:
        nf.fusion = L_.FUSE_AUTO


# ---- d. backward of both directions ------------------------------------------------------------------------------------------
def run_backward(tnf, g):
    p, z = g.params.cuda().requires_grad_(), g.z.cuda().requires_grad_()
    before = counts()
    out, ld = tnf.ops.coupling(z, p, g.D, g.L, g.U, g.upper, g.inverse)
    ((out * g.wz.cuda()).sum() + (ld * g.wl.cuda()).sum()).backward()
    return z.grad.cpu(), p.grad.cpu(), launched(before, BWD_FAMILIES)


def check_backward(tnf, sweep, g, route, group="backward", generic=True):
    """The default call on its expected route and the forced-generic call, counters in both directions."""
    L, what = g.L, g.what() + " " + route
    family = L_.DIAG_BWD_GENERIC if route == "generic" else L_.DIAG_BWD_WIDE
    gz, gp, ran = run_backward(tnf, g)
    assert ran == {family: 1}, (what, ran)
    name = "generic backward" if route == "generic" else group
    under(sweep, name + " g_z", L, gz, g.f64[0], what, WR.gerr)
    under(sweep, name + " g_params", L, gp, g.f64[1], what, WR.gerr)
    grad_err("wide sweep, %s backward: d params" % route, gp, g.f64[1])
    if generic:
        with forced_generic():
            fz, fp, ran = run_backward(tnf, g)
        assert ran == {L_.DIAG_BWD_GENERIC: 1}, (what, ran)
        under(sweep, "generic backward g_z", L, fz, g.f64[0], what, WR.gerr)
        under(sweep, "generic backward g_params", L, fp, g.f64[1], what, WR.gerr)
    return gz, gp


@pytest.mark.parametrize("D,L,U", WR.backward_shapes(), ids=[WR.bwd_id(*s) for s in WR.backward_shapes()])
def test_backward(tnf, sweep, D, L, U):
    """coupling_wide_bwd_kernel<HT, UT, L> + wide_gw_kernel<HT, UT> (the id names the cell and the family): one tile and
    three, and N = 1 -- one record, 127 empty pass-2 slices.  The cells the launcher refuses (LDS, the L limit) and
    per-context parameter rows run the generic kernel, asserted through its counter."""
    sweep.need("backward")
    HT, UT = WR.tiles(D, U)
    assert ((HT, UT, L) in WR.LDS_REFUSED_BWD) == (L <= (3 if UT <= 2 else 2) and not WR.wide_bwd_supported(D, L, U))
    for upper, inverse in WR.backward_direction(D, L, U):
        for M, Mp, N in WR.BWD_ROWS:
            check_backward(tnf, sweep, sweep.bwd[(D, L, U, upper, inverse, M, Mp, N)], WR.backward_route(D, L, U, Mp, N))


@pytest.mark.parametrize("N", WR.SLICE_NS, ids=["%s-N%d-wide" % (WR.case_id(*WR.SLICE_CELL), N) for N in WR.SLICE_NS])
def test_backward_slicing(tnf, sweep, N):
    """Pass 2 with fewer tiles than 128 x the slice length (empty slices, a ragged last one) and pass 1 with more tiles
    than waves (2,050 on 512 workgroups: a second tile, the last one ragged); no atomics anywhere: two runs agree bit
    for bit."""
    sweep.need("slicing")
    per, used, last = WR.slicing(N)
    assert used < WR.SLICES and (last < per or N == 2065)
    assert WR.tiles_per_wave(N, WR.bwd_bx(N)) == (2 if N > 32768 else 1)
    g = sweep.slices[N]
    gz, gp = check_backward(tnf, sweep, g, "wide", group="sliced backward", generic=False)
    gz2, gp2, ran = run_backward(tnf, g)
    assert ran == {L_.DIAG_BWD_WIDE: 1} and torch.equal(gz, gz2) and torch.equal(gp, gp2)


# ---- e. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,S,L,U", WR.TRAIN_SHAPES, ids=["D%d-S%d-L%d-U%d-bijectors-wide" % s for s in WR.TRAIN_SHAPES])
def test_flow_log_prob_backward(tnf, sweep, D, S, L, U):
    """NormFlow.log_prob under autograd at a wide shape: no fused training pair exists, so the per-bijector composition
    runs, each of its 2 S RealNVP layers backward through the two-pass wide kernels."""
    sweep.need("train")
    t = sweep.train[(D, S, L, U)]
    nf = t.flow.nf
    p, z = t.flow.params.cuda().requires_grad_(), t.zin.cuda()
    assert nf._route("log_prob", z, p) == ("bijectors", False, False)
    before = counts()
    nf.log_prob(z, p).sum().backward()
    ran = launched(before, BWD_FAMILIES)
    assert ran == {L_.DIAG_BWD_WIDE: 2 * S}, ran
    under(sweep, "unfused flow backward g_params", L, p.grad.cpu(), t.g64, "flow D%d backward" % D, WR.gerr)
