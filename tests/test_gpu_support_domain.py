"""ToInterval and ToSimplex over their own domain, standalone (support_kernels.hip) and fused (support_math.h:
interval_fast, the load / store stage of the one-kernel flow paths), against the CPU oracle in float64 -- in the pattern
of tests/test_gpu_cond_domain.py and tests/test_gpu_mog.py.  Helpers: tests/support_restatement.py; the host half, which
pins the noise model without a GPU: tests/test_support_host.py.

Reference: oracle/flow_oracle.py: to_interval / to_simplex under domain_helpers.float64(), on the kernel's float32 inputs
and float32 constants (interval_consts rounds them as the (7, D) block does).  Error: max |got - want| / max(1, max
|want|); gradients through conftest.grad_err.  Inputs (fixed, well-conditioned): ToInterval z ~ N(0, 1) clamped to +-2.5,
bounds multiples of 1/8 with half-widths in [0.5, 3], the inverse's input the float32 oracle's forward image, every case
asserting 1 - |u| >= 0.01 on tanh and |x - c| >= 0.05 on softplus features; ToSimplex z ~ N(-1, 1).

A, B  standalone, float32 and float64, values, log-dets and autograd gradients, D (Din) in 1, 2, 3, 5, 17, 31, 32, 33,
      64, 127, 257, 1000, 5000 with the feature kind by d % 4, the four one-kind patterns at D = 5 and 33 (identity
      features bit-equal, exactly 0 in the log-det), rows at 1, R - 1, R, R + 1, 2R + 1 of the launcher's rows_per_block
      laid out (1, rows), (rows, 1), (3, .), both D_attr of ToSimplex, and the 64 KB LDS bound: the widest accepted row
      per dtype meets the oracle, one wider is refused with nothing launched (ToSimplex backward has its own bound).
      float32 bar: 4 x the float32 oracle's own error against float64 over these cases (guarded to 1e-9 .. 1e-5);
      float64 bar: rtol = atol = 1e-11.  Saturation (|z| = 10, 30 on tanh) and the softplus threshold (z = -90 .. 30)
      are a test of their own, tanh against the float32 oracle since there the precisions differ by construction.
C     the fused stage on every route that has one -- flow_fused2, flow_fused3, flow_fused_f16 (D = 64, 32; S = 1, 4 and
      a shape flow_fused2 refuses), the range chain's support arm (layer variants 10 and 12), the AR one-kernel paths
      (D = 2, 5, 21, 33, 64: padded strides) and ar_train parameter gradients (D = 5, 21, 32) -- against the float64
      composition, (M_z, M_p, N) in (1,1,1), (1,1,17), (3,3,529), (3,1,529), exactly one launch of the expected family
      and none of another; and one case each of the routes that do not fuse (padded, FUSE_LAYER, ToSimplex).
      Bars: the suite's bar of the route without a support layer (domain_helpers.py) with atol raised by 4 x the absolute
      error, on the case's inputs, of interval_fast restated in float32 against float64 -- per element for z, per row of
      log-det for log_prob, log_q and sum_log_det; every fused case prints these four errors when it is built.  No bar
      comes from a kernel's output.

When the module is done it prints the largest error per bar as a fraction of the bar.  Measured on the MI355X (oracle
noise 5.1e-7 values, 1.8e-6 gradients; ToSimplex 1.4e-7, 2.5e-7): standalone ToInterval float32 forward values 0.05,
log-det 0.29, gradient 0.02, inverse values 0.27, log-det 0.45, gradient 0.28; ToSimplex float32 values 0.15, log-det
0.31, gradient 0.26; float64 at or below 0.01 of 1e-11 away from saturation.  Fused: log_prob 0.04 (flow_fused2,
flow_fused3), 0.03 (flow_fused_f16, range chain), 0.09 (AR); sampled z 0.30 (flow_fused2), 0.10 (flow_fused_f16), 0.04
(AR); log_q 0.03 .. 0.06; z0 and sum_log_det at most 0.02; ar_train d params 0.03; unfused routes at most 0.08.
Before the row sums of support_kernels.hip accumulated in double the sweep failed at ToInterval D = 16383 (log-det 1.15
of the bar) and ToSimplex Din = 5000, 8190 (gradient 1.6, 2.2 of the bar)."""
import numpy as np
import pytest
import torch

import support_restatement as SR
from conftest import grad_err
from domain_helpers import (BAR_P, FORWARD_FAMILIES, INV_TOL, LOGP_TOL, LQ_TOL, SLDF_TOL, ZF_TOL, counts, float64,
                            launched, variants)
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib
F64_TOL = dict(rtol=1e-11, atol=1e-11)  # tests/test_gpu_support.py: tol


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


_WORST = {}  # quantity -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error, %s: %.3f of the bar" % (name, frac))


def note(name, frac):
    _WORST[name] = max(frac, _WORST.get(name, 0.0))


def within(name, got, want, what, rtol, atol):
    """torch.testing.assert_close, after noting the largest |got - want| / (atol + rtol |want|) under `name`."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    note(name, float(((got - want).abs() / (atol + rtol * want.abs())).max()))
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda s: "%s, %s: %s" % (name, what, s))


def under(name, got, want, bar, what):
    """The standalone float32 comparison: SR.err against `bar`."""
    e = SR.err(got, want)
    note(name, e / bar)
    assert bool(torch.isfinite(got).all()) and e <= bar, "%s, %s: error %.3e exceeds %.3e" % (name, what, e, bar)


def raised(tol, e):
    return dict(rtol=tol["rtol"], atol=tol["atol"] + 4.0 * e)


def print_raise(what, e):
    """The restatement's absolute errors of one fused case; each fused bar's atol is its route's plus 4 x one of these."""
    print("fused bars, %s: restated interval_fast against float64: sampled z %.3e, its log-det per row %.3e, recovered z "
          "%.3e, its log-det per row %.3e; atol + 4 x these" % (what, e["fz"], e["fl"], e["iz"], e["il"]))


def layouts(r):
    """(M, N) of a call on r rows, and one on about r rows with neither dimension 1."""
    return [(1, r), (r, 1), (3, r // 3 + 1)]


def max_rows(R):
    return max(3 * (r // 3 + 1) for r in SR.row_edges(R))


# ---- A. standalone ToInterval -------------------------------------------------------------------------------------------
INTERVAL_CASES = [(D, "mixed") for D in SR.D_LIST] + [(D, p) for D in (5, 33) for p in SR.KINDS]


def interval_case(oracle, D, pattern, _cache={}):
    """Rows for the smaller R of the two dtypes' tilings are a subset of the float32 case's: one case per (D, pattern)."""
    if (D, pattern) not in _cache:
        _cache[(D, pattern)] = SR.IntervalCase(oracle, D, pattern, max_rows(SR.rows_per_block(D, 4, 1)))
    return _cache[(D, pattern)]


@pytest.fixture(scope="module")
def interval_bars(oracle):
    """4 x the float32 oracle's error against the float64 oracle over the sweep's cases, the LDS-limit rows included."""
    cs = [interval_case(oracle, D, p) for D, p in INTERVAL_CASES] + [SR.IntervalCase(oracle, SR.max_width(4, False), "mixed", 3)]
    v, g = max(c.noise()[0] for c in cs), max(c.noise()[1] for c in cs)
    print("ToInterval float32 oracle noise: values and log-dets %.3e, gradients %.3e -> bars %.3e, %.3e" % (v, g, 4 * v, 4 * g))
    assert 1e-9 < v < 1e-5 and 1e-9 < g < 1e-5
    return 4.0 * v, 4.0 * g


def run_interval(tnf, c, dt, inverse, rows, M, N, bars, what):
    """One standalone call and its backward on the first `rows` rows of the case, laid out (M, N)."""
    n = M * N
    assert n <= c.rows
    inp = (c.x if inverse else c.z)[0, :n].reshape(M, N, c.D).to(dt).cuda().requires_grad_()
    out, ld = tnf.ops.to_interval(inp, c.c7.cuda(), inverse)
    wz, wl = c.wz[0, :n].reshape(M, N, c.D).to(dt).cuda(), c.wl[0, :n].reshape(M, N).to(dt).cuda()
    ((out * wz).sum() + (ld * wl).sum()).backward()
    assert out.shape == (M, N, c.D) and ld.shape == (M, N) and out.dtype == ld.dtype == inp.grad.dtype == dt
    w_out, w_ld, w_g = (t[0, :n] for t in c.ref64[inverse])
    got = (out.detach().reshape(n, c.D).cpu(), ld.detach().reshape(n).cpu(), inp.grad.reshape(n, c.D).cpu())
    idt = c.kind == 3
    assert torch.equal(got[0][:, idt], inp.detach().reshape(n, c.D).cpu()[:, idt]), "%s: identity features changed" % what
    if c.pattern == "identity":
        assert bool((got[1] == 0).all()), "%s: identity features add to the log-det" % what
    d = "inverse" if inverse else "forward"
    if dt == torch.float64:
        for name, a, b in (("values", got[0], w_out), ("log-det", got[1], w_ld), ("gradient", got[2], w_g)):
            within("ToInterval float64 %s" % name, a, b, what, **F64_TOL)
    else:
        under("ToInterval float32 %s values" % d, got[0], w_out, bars[0], what)
        under("ToInterval float32 %s log-det" % d, got[1], w_ld, bars[0], what)
        note("ToInterval float32 %s gradient" % d, SR.gerr(got[2], w_g) / bars[1])
        grad_err("support sweep, ToInterval %s: d z" % d, got[2], w_g, bars[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D,pattern", INTERVAL_CASES, ids=["D%d-%s" % c for c in INTERVAL_CASES])
def test_interval_standalone(tnf, oracle, interval_bars, D, pattern, dt):
    """Rows on every edge of the launcher's tiling R (recomputed here for this D and dtype), three layouts each."""
    c = interval_case(oracle, D, pattern)
    R = SR.rows_per_block(D, dt.itemsize, 1)
    assert R == 1 or D < 5000
    for inverse in (False, True):
        for r in SR.row_edges(R):
            for M, N in layouts(r):
                run_interval(tnf, c, dt, inverse, r, M, N, interval_bars, "D%d %s R%d (%d, %d) inverse=%d" % (D, pattern, R, M, N, inverse))


def _raw_interval(c7d, inp, out, ld, inverse):
    M, N, D = inp.shape
    return lib.tnf_to_interval(L_.F64 if inp.dtype == torch.float64 else L_.F32, inp.data_ptr(), c7d.data_ptr(), out.data_ptr(),
                               ld.data_ptr(), M * N, D, int(inverse), L_.stream_ptr())


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_interval_lds_limit(tnf, oracle, interval_bars, dt):
    """(D + 1) esz <= 64 KB at R = 1: three rows at the widest accepted D meet the oracle in both directions; one feature
    more is refused with the library's error before anything is launched (the outputs keep their fill)."""
    D = SR.max_width(dt.itemsize, False)
    assert SR.rows_per_block(D, dt.itemsize, 1) == 1
    c = SR.IntervalCase(oracle, D, "mixed", 3)
    for inverse in (False, True):
        run_interval(tnf, c, dt, inverse, 3, 1, 3, interval_bars, "D%d at the LDS limit, inverse=%d" % (D, inverse))
    lb, ub = SR.bounds(D + 1)
    c7d = SR.consts7(oracle.interval_consts(lb, ub)).cuda()
    inp = torch.zeros(1, 3, D + 1, dtype=dt, device="cuda")
    out, ld = torch.full_like(inp, 7.0), torch.full((1, 3), 7.0, dtype=dt, device="cuda")
    for inverse in (False, True):
        assert _raw_interval(c7d, inp, out, ld, inverse) == L_.EUNSUPPORTED
        assert "LDS" in lib.tnf_last_error().decode()
        with pytest.raises(L_.TnfError, match="to_interval: D=%d" % (D + 1)):
            tnf.ops.to_interval(inp, c7d, inverse)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ld == 7.0).all())


def test_interval_saturation_and_threshold(tnf, oracle, interval_bars):
    """Saturated tanh and the softplus threshold branch.  tanh at |z| = 10, 30: float32 tanh is exactly +-1, so out is
    +-tanh_m + tanh_c exactly and the log-det log tanh_m + log(1e-12) to float32 rounding (4 ulp: the float32 log of the
    constant, its sum with the constant row) -- compared with the float32 oracle, since float64 does not saturate at 10.
    softplus at z = -90 .. 30 against float64 at the standalone bar, out = z m + c exactly above the threshold 20.
    Gradients finite everywhere; the float64 kernel meets the float64 oracle at 1e-11 on the same points."""
    # tanh: D = 1, one point per row
    lb, ub = np.array([-0.75]), np.array([2.5])
    consts = oracle.interval_consts(lb, ub)
    c7d = SR.consts7(consts).cuda()
    zt = torch.tensor([10.0, -10.0, 30.0, -30.0]).reshape(1, 4, 1)
    tm, tc = float(consts[2]), float(consts[3])
    with torch.no_grad():
        o32, l32 = oracle.to_interval(zt, consts, False)
    zr = zt.cuda().requires_grad_()
    out, ld = tnf.ops.to_interval(zr, c7d, False)
    (out.sum() + ld.sum()).backward()
    assert torch.equal(out.detach().cpu(), torch.sign(zt) * tm + tc) and torch.equal(out.detach().cpu(), o32)
    want_ld = np.log(np.float32(tm)) + np.log(np.float32(1e-12))
    torch.testing.assert_close(ld.detach().cpu(), torch.full((1, 4), float(want_ld)), rtol=4 * 1.2e-7, atol=0)
    torch.testing.assert_close(ld.detach().cpu(), l32, rtol=4 * 1.2e-7, atol=0)
    assert bool(torch.isfinite(zr.grad).all())
    # softplus: D = 2 (lower bound, upper bound), one point per row
    lb2, ub2 = np.array([0.375, -np.inf]), np.array([np.inf, -1.25])
    consts2 = oracle.interval_consts(lb2, ub2)
    c7d2 = SR.consts7(consts2).cuda()
    pts = torch.tensor([-90.0, -30.0, 19.5, 20.0, 20.5, 30.0])
    zs = pts[None, :, None].repeat(1, 1, 2).contiguous()
    with torch.no_grad(), float64():
        o64, l64 = oracle.to_interval(zs.double(), consts2, False)
    zr = zs.cuda().requires_grad_()
    out, ld = tnf.ops.to_interval(zr, c7d2, False)
    (out.sum() + ld.sum()).backward()
    print("softplus threshold points: values %.3e, log-det %.3e (bar %.3e)" % (SR.err(out, o64), SR.err(ld, l64), interval_bars[0]))
    under("ToInterval float32 threshold values", out.detach().cpu(), o64, interval_bars[0], "softplus points")
    under("ToInterval float32 threshold log-det", ld.detach().cpu(), l64, interval_bars[0], "softplus points")
    above = pts > 20
    m, cc = consts2[4].reshape(-1), consts2[5].reshape(-1)
    assert torch.equal(out.detach().cpu()[0, above], zs[0, above] * m + cc)
    assert bool(torch.isfinite(zr.grad).all())
    # float64 kernel against the float64 oracle on the same points
    for z, cs, cd in ((zt, consts, c7d), (zs, consts2, c7d2)):
        with float64():
            zo = z.double().requires_grad_()
            o, l = oracle.to_interval(zo, cs, False)
            (o.sum() + l.sum()).backward()
        zr = z.double().cuda().requires_grad_()
        out, ld = tnf.ops.to_interval(zr, cd, False)
        (out.sum() + ld.sum()).backward()
        print("float64 on the saturation / threshold points: values %.3e log-det %.3e gradient %.3e" %
              (SR.abs_err(out, o), SR.abs_err(ld, l), SR.abs_err(zr.grad, zo.grad)))
        within("ToInterval float64 values", out, o.detach(), "saturation points", **F64_TOL)
        within("ToInterval float64 log-det", ld, l.detach(), "saturation points", **F64_TOL)
        within("ToInterval float64 gradient", zr.grad, zo.grad, "saturation points", **F64_TOL)


# ---- B. standalone ToSimplex --------------------------------------------------------------------------------------------
def simplex_case(oracle, Din, D_attr, _cache={}):
    if (Din, D_attr) not in _cache:
        R = min(SR.rows_per_block(Din, 4, 1), 256)
        _cache[(Din, D_attr)] = SR.SimplexCase(oracle, Din, D_attr, max_rows(R))
    return _cache[(Din, D_attr)]


@pytest.fixture(scope="module")
def simplex_bars(oracle):
    cs = [simplex_case(oracle, Din, Din + a) for Din in SR.D_LIST for a in (0, 1)]
    cs += [SR.SimplexCase(oracle, SR.max_width(4, b), SR.max_width(4, b), 3) for b in (False, True)]
    v, g = max(c.noise()[0] for c in cs), max(c.noise()[1] for c in cs)
    print("ToSimplex float32 oracle noise: values and log-dets %.3e, gradients %.3e -> bars %.3e, %.3e" % (v, g, 4 * v, 4 * g))
    assert 1e-9 < v < 1e-5 and 1e-9 < g < 1e-5
    return 4.0 * v, 4.0 * g


def run_simplex(tnf, c, dt, M, N, bars, what, backward=True):
    n = M * N
    assert n <= c.rows
    inp = c.z[0, :n].reshape(M, N, c.Din).to(dt).cuda().requires_grad_()
    out, ld = tnf.ops.to_simplex(inp, c.D_attr)
    assert out.shape == (M, N, c.Din + 1) and ld.shape == (M, N) and out.dtype == ld.dtype == dt
    torch.testing.assert_close(out.detach().sum(2).cpu(), torch.ones(M, N, dtype=dt), rtol=1e-5, atol=1e-5)
    wz, wl = c.wz[0, :n].reshape(M, N, c.Din + 1).to(dt).cuda(), c.wl[0, :n].reshape(M, N).to(dt).cuda()
    loss = (out * wz).sum() + (ld * wl).sum()
    w_out, w_ld, w_g = (t[0, :n] for t in c.ref64)
    got = [out.detach().reshape(n, c.Din + 1).cpu(), ld.detach().reshape(n).cpu()]
    if dt == torch.float64:
        within("ToSimplex float64 values", got[0], w_out, what, **F64_TOL)
        within("ToSimplex float64 log-det", got[1], w_ld, what, **F64_TOL)
    else:
        under("ToSimplex float32 values", got[0], w_out, bars[0], what)
        under("ToSimplex float32 log-det", got[1], w_ld, bars[0], what)
    if not backward:  # past the backward kernel's own LDS bound: the library's refusal
        with pytest.raises(L_.TnfError, match="to_simplex_backward: D=%d" % c.Din):
            loss.backward()
        return
    loss.backward()
    g = inp.grad.reshape(n, c.Din).cpu()
    if dt == torch.float64:
        within("ToSimplex float64 gradient", g, w_g, what, **F64_TOL)
    else:
        note("ToSimplex float32 gradient", SR.gerr(g, w_g) / bars[1])
        grad_err("support sweep, ToSimplex: d z", g, w_g, bars[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("Din", SR.D_LIST)
def test_simplex_standalone(tnf, oracle, simplex_bars, Din, dt):
    """Rows on the edges of the forward kernel's R and of the backward kernel's own (three planes), three layouts each,
    D_attr = Din and Din + 1.  Din = 5000 in float64 is past the backward's bound (4094): forward checked, backward refused."""
    esz = dt.itemsize
    edges = sorted(set(SR.row_edges(SR.rows_per_block(Din, esz, 1)) + SR.row_edges(SR.rows_per_block(Din, esz, 3))))
    backward = SR.lds_bytes(Din, esz, True) <= SR.LDS_LIMIT
    assert backward == ((Din, esz) != (5000, 8))
    for a in (0, 1):
        c = simplex_case(oracle, Din, Din + a)
        for r in edges:
            for M, N in layouts(r):
                run_simplex(tnf, c, dt, M, N, simplex_bars, "Din%d D_attr%d (%d, %d)" % (Din, Din + a, M, N), backward)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_simplex_lds_limits(tnf, oracle, simplex_bars, dt):
    """Forward: (Din + 1) esz <= 64 KB; backward: (2 (Din + 1) + 1) esz <= 64 KB.  Three rows at each limit meet the
    oracle; one feature more is refused by that kernel with nothing launched."""
    esz = dt.itemsize
    Df, Db = SR.max_width(esz, False), SR.max_width(esz, True)
    run_simplex(tnf, SR.SimplexCase(oracle, Db, Db, 3), dt, 1, 3, simplex_bars, "Din%d at the backward LDS limit" % Db)
    run_simplex(tnf, SR.SimplexCase(oracle, Db + 1, Db + 1, 3), dt, 1, 3, simplex_bars, "Din%d past it" % (Db + 1), backward=False)
    run_simplex(tnf, SR.SimplexCase(oracle, Df, Df, 3), dt, 1, 3, simplex_bars, "Din%d at the forward LDS limit" % Df, backward=False)
    code = L_.F64 if dt == torch.float64 else L_.F32
    inp = torch.zeros(1, 3, Df + 1, dtype=dt, device="cuda")
    out, ld = torch.full((1, 3, Df + 2), 7.0, dtype=dt, device="cuda"), torch.full((1, 3), 7.0, dtype=dt, device="cuda")
    assert lib.tnf_to_simplex(code, inp.data_ptr(), out.data_ptr(), ld.data_ptr(), 3, Df + 1, Df + 1, L_.stream_ptr()) == L_.EUNSUPPORTED
    assert "to_simplex: D=%d" % (Df + 1) in lib.tnf_last_error().decode()
    gz = torch.full((1, 3, Db + 1), 7.0, dtype=dt, device="cuda")
    assert lib.tnf_to_simplex_backward(code, inp.data_ptr(), out.data_ptr(), ld.data_ptr(), gz.data_ptr(), 3, Db + 1, Db + 1,
                                       L_.stream_ptr()) == L_.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ld == 7.0).all()) and bool((gz == 7.0).all())


# ---- C. the fused ToInterval stage --------------------------------------------------------------------------------------
MNS = [(1, 1, 1), (1, 1, 17), (3, 3, 529), (3, 1, 529)]
M_FULL, N_FULL = 3, 529


class CouplingCase:
    """A coupling flow with a mixed-bounds ToInterval on top, at the ops level: parameters, frozen statistics, a base draw
    of (3, 529) rows; per M_p in (3, 1) the float64 composition both ways and the restatement's absolute errors on that
    case's inputs.  Every smaller (M_z, M_p, N) is a slice: the flow is row-wise."""

    def __init__(self, oracle, D, S, L, U, seed):
        self.dims = (D, S, L, U)
        g = torch.Generator().manual_seed(seed)
        P = lib.tnf_flow_num_params(D, S, L, U)
        self.params = torch.randn(M_FULL, P, generator=g) * 0.02
        self.mean = torch.randn(2 * S, D, generator=g) * 0.05
        self.alpha = torch.rand(2 * S, D, generator=g) * 0.1 + 0.95
        self.omega = torch.randn(M_FULL, N_FULL, D, generator=g).clamp_(-1.5, 1.5)  # the core's output stays within +-2.6
        self.lb, self.ub = SR.bounds(D)
        self.consts = oracle.interval_consts(self.lb, self.ub)
        self.c7 = SR.consts7(self.consts)
        stats64 = [(m.double(), a.double()) for m, a in zip(self.mean, self.alpha)]
        self.ref = {}
        for Mp in (M_FULL, 1):
            p64 = self.params[:Mp].double()
            with torch.no_grad(), float64():
                zc, lqc, _ = oracle.flow_forward(self.omega.double().numpy(), p64, D, S, L, U, stats64)
                x, ldf = oracle.to_interval(zc, self.consts, False)
                lq = lqc - ldf
                base = torch.tensor(oracle.base_log_density_f64(self.omega.double().numpy()))
                xin = x.float()  # the log_prob direction's input
                zi, ldi = oracle.to_interval(xin.double(), self.consts, True)
                z0, sld = oracle.flow_inverse(zi, p64, D, S, L, U, stats64)
                lp = oracle.flow_log_prob(zi, p64, D, S, L, U, stats64) - ldi
            assert x.dtype == lq.dtype == lp.dtype == torch.float64
            SR.assert_conditioned(xin, self.consts)
            assert float(zc.abs().max()) <= 2.6, "the support stage's input left the sweep's domain"
            # the restatement's absolute error on this case's inputs, per direction
            fo, fl = SR.restated(zc.float(), self.c7, False)
            io, il = SR.restated(xin, self.c7, True)
            e = dict(fz=SR.abs_err(fo, x), fl=SR.abs_err(fl, ldf), iz=SR.abs_err(io, zi), il=SR.abs_err(il, ldi))
            assert all(1e-9 < v < 1e-4 for v in e.values()), e
            print_raise("coupling D%d S%d M_p%d" % (D, S, Mp), e)
            self.ref[Mp] = dict(x=x, lq=lq, sldf=base - lq, xin=xin, z0=z0, sld=sld + ldi, lp=lp, e=e)


_COUPLING = {}


def coupling_case(oracle, D, S):
    if (D, S) not in _COUPLING:
        _COUPLING[(D, S)] = CouplingCase(oracle, D, S, 2, 15, 100 * D + S)
    return _COUPLING[(D, S)]


def one_launch(before, family):
    ran = launched(before, FORWARD_FAMILIES)
    assert ran == {family: 1}, (ran, family)


def check_coupling(tnf, c, fv, fam_inv, fam_fwd):
    D, S, L, U = c.dims
    dev = L_.require_device()
    mean, alpha, c7d = c.mean.to(dev), c.alpha.to(dev), c.c7.to(dev)
    for Mz, Mp, N in MNS:
        r = c.ref[M_FULL if Mp == M_FULL else 1]
        e = r["e"]
        what = "D%d S%d variant %d (%d, %d, %d)" % (D, S, fv, Mz, Mp, N)
        p = c.params[:Mp].to(dev)
        with variants(flow=fv), torch.no_grad():
            before = counts()
            lp, z0, sld = tnf.ops.flow_log_prob_raw(r["xin"][:Mz, :N].to(dev), p, mean, alpha, D, S, L, U, L_.FUSE_FLOW,
                                                    want_z0=True, want_sld=True, interval_consts=c7d)
            one_launch(before, fam_inv)
            om = c.omega[:Mz, :N].to(dev)
            before = counts()
            z, sldf = tnf.ops.flow_forward_raw(om, p, mean, alpha, D, S, L, U, L_.FUSE_FLOW, interval_consts=c7d)
            one_launch(before, fam_fwd)
            before = counts()
            z2, sldf2, lq2 = tnf.ops.flow_forward_raw(om, p, mean, alpha, D, S, L, U, L_.FUSE_FLOW, interval_consts=c7d,
                                                      want_log_q=True)
            one_launch(before, fam_fwd)
        fam = {L_.DIAG_FLOW_FUSED2: "flow_fused2", L_.DIAG_FLOW_FUSED3: "flow_fused3", L_.DIAG_FLOW_F16: "flow_fused_f16"}[fam_inv]
        within("%s log_prob" % fam, lp, r["lp"][:Mz, :N], what, **raised(LOGP_TOL, e["il"]))
        within("%s z0" % fam, z0, r["z0"][:Mz, :N], what, **raised(INV_TOL, e["iz"]))
        within("%s sum_log_det" % fam, sld, r["sld"][:Mz, :N], what, **raised(INV_TOL, e["il"]))
        famf = "flow_fused2" if fam_fwd == L_.DIAG_FLOW_FUSED2_FWD else "flow_fused_f16"
        base = tnf.ops.base_log_density_f64(om.double())
        within("%s sampled z" % famf, z, r["x"][:Mz, :N], what, **raised(ZF_TOL, e["fz"]))
        within("%s forward sum_log_det" % famf, sldf, r["sldf"][:Mz, :N], what, **raised(SLDF_TOL, e["fl"]))
        within("%s log_q" % famf, base - sldf, r["lq"][:Mz, :N], what, **raised(LQ_TOL, e["fl"]))
        assert torch.equal(z2, z) and torch.equal(sldf2, sldf)
        if fam_fwd == L_.DIAG_FLOW_FUSED2_FWD:  # the kernel writes log_q (float64) itself, from the float32 draw
            assert lq2 is not None and lq2.dtype == torch.float64
            within("flow_fused2 log_q, written by the kernel", lq2, r["lq"][:Mz, :N], what, **raised(LQ_TOL, e["fl"]))
        else:
            assert lq2 is None


@pytest.mark.parametrize("fv", [10, 20, 15])
@pytest.mark.parametrize("D,S", [(64, 1), (64, 4), (32, 1), (32, 4)])
def test_fused_coupling(tnf, oracle, D, S, fv):
    """TNF_OPT_FLOW_VARIANT 10: flow_fused2 both ways; 20: flow_fused3 on the inverse (sampling has none: flow_fused2);
    15: flow_fused_f16 both ways."""
    assert lib.tnf_flow_fused2_supported(D, S, 2, 15) and lib.tnf_flow_fused3_supported(D, S, 2, 15)
    fam_inv = {10: L_.DIAG_FLOW_FUSED2, 20: L_.DIAG_FLOW_FUSED3, 15: L_.DIAG_FLOW_F16}[fv]
    check_coupling(tnf, coupling_case(oracle, D, S), fv, fam_inv, L_.DIAG_FLOW_F16 if fv == 15 else L_.DIAG_FLOW_FUSED2_FWD)


def test_fused_coupling_refused_by_flow_fused2(tnf, oracle):
    """D = 64, S = 7, L = 2: the whole flow fits flow_fused_f16 but not flow_fused2, so variant 10 lands in flow_fused_f16."""
    D, S = 64, 7
    assert lib.tnf_flow_fused_supported(D, S, 2, 15) and not lib.tnf_flow_fused2_supported(D, S, 2, 15)
    check_coupling(tnf, coupling_case(oracle, D, S), 10, L_.DIAG_FLOW_F16, L_.DIAG_FLOW_F16)


@pytest.mark.parametrize("lv", [10, 12])
def test_range_chain_support_arm(tnf, oracle, lv):
    """FUSE_LAYER with layer variant >= 10: the range chain evaluates ToInterval^-1 in its first launch (NormFlow never
    gets here: its per-layer route does not fuse).  Layer variant 0 has no such arm: EUNSUPPORTED from select_flow_kernel."""
    D, S, L, U = 64, 4, 2, 15
    c = coupling_case(oracle, D, S)
    dev = L_.require_device()
    r = c.ref[M_FULL]
    e = r["e"]
    args = (r["xin"].to(dev), c.params.to(dev), c.mean.to(dev), c.alpha.to(dev), D, S, L, U, L_.FUSE_LAYER)
    per = max(lv - 10, 1)
    with variants(layer=lv), torch.no_grad():
        before = counts()
        lp, z0, sld = tnf.ops.flow_log_prob_raw(*args, want_z0=True, want_sld=True, interval_consts=c.c7.to(dev))
        ran = launched(before, FORWARD_FAMILIES)
    assert ran == {L_.DIAG_FLOW_RANGE2: (2 * S + per - 1) // per}, ran
    what = "D64 S4 layer variant %d" % lv
    within("range chain log_prob", lp, r["lp"], what, **raised(LOGP_TOL, e["il"]))
    within("range chain z0", z0, r["z0"], what, **raised(INV_TOL, e["iz"]))
    within("range chain sum_log_det", sld, r["sld"], what, **raised(INV_TOL, e["il"]))
    with variants(layer=0), torch.no_grad():
        before = counts()
        with pytest.raises(L_.TnfError, match="a fused support layer needs the whole-flow kernel"):
            tnf.ops.flow_log_prob_raw(*args, interval_consts=c.c7.to(dev))
        assert launched(before, FORWARD_FAMILIES) == {}


class ArCase:
    """NormFlow('AR', support_layer=ToInterval) with mixed bounds and frozen statistics; the float64 composition both ways
    on (3, 529) rows per M_p, as CouplingCase."""

    def __init__(self, tnf, oracle, D, L=2, U=15):
        np.random.seed(D)
        torch.manual_seed(D)
        self.D, self.L, self.U = D, L, U
        self.lb, self.ub = SR.bounds(D)
        self.nf = tnf.NormFlow(D, True, "AR", 1, L, U, tnf.ToInterval(D, self.lb, self.ub))
        g = torch.Generator().manual_seed(D + 5)
        mean, alpha = torch.randn(D, generator=g) * 0.05, torch.rand(D, generator=g) * 0.1 + 0.95
        self.nf.bijectors[1].set_last_stats(mean, alpha)
        self.params = torch.randn(M_FULL, self.nf.D_params, generator=g) * 0.05
        self.omega = torch.randn(M_FULL, N_FULL, D, generator=g).clamp_(-1.5, 1.5)
        self.consts = oracle.interval_consts(self.lb, self.ub)
        self.c7 = SR.consts7(self.consts)
        assert torch.equal(self.c7, self.nf.bijectors[-1]._consts)
        self.Ms = [Mk[0].numpy() for Mk in self.nf.bijectors[0].Ms]
        self.stat = (mean.double(), alpha.double())
        self.w = torch.rand(M_FULL, N_FULL, generator=g) * 0.8 + 0.2
        self.oracle = oracle
        n_maf = oracle.maf_num_params(D, L, U)
        self.ref = {}
        for Mp in (M_FULL, 1):
            p64 = self.params[:Mp].double()
            with torch.no_grad(), float64():
                om = self.omega.double()
                lq = torch.tensor(oracle.base_log_density_f64(om.numpy()))
                z, ld = oracle.maf(om, p64[:, :n_maf], D, L, U, self.Ms, False)
                lq = lq - ld
                z, ld = oracle.bn_forward_frozen(z, *self.stat)
                lq = lq - ld
                zc, ld = oracle.affine(z, p64[:, n_maf:n_maf + 2 * D], D, False)
                lq = lq - ld
                x, ldf = oracle.to_interval(zc, self.consts, False)
                lq = lq - ldf
                xin = x.float()
                zi, ldi = oracle.to_interval(xin.double(), self.consts, True)
                lp = oracle.ar_flow_log_prob(zi, p64, D, L, U, self.Ms, self.stat) - ldi
            assert x.dtype == lq.dtype == lp.dtype == torch.float64
            SR.assert_conditioned(xin, self.consts)
            assert float(zc.abs().max()) <= 2.6, "the support stage's input left the sweep's domain"
            fo, fl = SR.restated(zc.float(), self.c7, False)
            io, il = SR.restated(xin, self.c7, True)
            e = dict(fz=SR.abs_err(fo, x), fl=SR.abs_err(fl, ldf), iz=SR.abs_err(io, zi), il=SR.abs_err(il, ldi))
            assert all(1e-9 < v < 1e-4 for v in e.values()), e
            print_raise("AR D%d M_p%d" % (D, Mp), e)
            self.ref[Mp] = dict(x=x, lq=lq, xin=xin, lp=lp, e=e)

    def ref_grad(self, Mp):
        """d loss / d params of loss = -(w log_prob).sum() / N by torch autograd over the float64 composition."""
        pr = self.params[:Mp].double().requires_grad_()
        with float64():
            zi, ldi = self.oracle.to_interval(self.ref[Mp]["xin"].double(), self.consts, True)
            lp = self.oracle.ar_flow_log_prob(zi, pr, self.D, self.L, self.U, self.Ms, self.stat) - ldi
            (-(lp * self.w.double()).sum() / N_FULL).backward()
        return pr.grad


_AR = {}


def ar_case(tnf, oracle, D):
    if D not in _AR:
        _AR[D] = ArCase(tnf, oracle, D)
    return _AR[D]


@pytest.mark.parametrize("D", [2, 5, 21, 33, 64])
def test_fused_ar(tnf, oracle, D):
    """The AR one-kernel paths (maf_mfma.hip): constants indexed by the padded stride DP > D, a constant row next to the
    padded tail.  log_prob and the frozen forward through NormFlow; no coupling family launches."""
    c = ar_case(tnf, oracle, D)
    nf = c.nf
    for Mz, Mp, N in MNS:
        r = c.ref[M_FULL if Mp == M_FULL else 1]
        e = r["e"]
        what = "AR D%d (%d, %d, %d)" % (D, Mz, Mp, N)
        p = c.params[:Mp].cuda()
        xin, om = r["xin"][:Mz, :N].cuda(), c.omega[:Mz, :N].cuda()
        with torch.no_grad():
            assert nf._route("log_prob", xin, p) == ("ar_fused", True, False)
            assert nf._route("forward", om, p, True) == ("ar_fused", True, False)  # maf_mfma's forward has no launch counter
            before = counts()
            lp = nf.log_prob(xin, p)
            z, lq = nf._forward_from(om.double(), p, freeze_bn=True)
            assert launched(before, FORWARD_FAMILIES) == {}
        within("AR log_prob", lp, r["lp"][:Mz, :N], what, **raised(LOGP_TOL, e["il"]))
        within("AR sampled z", z, r["x"][:Mz, :N], what, **raised(ZF_TOL, e["fz"]))
        within("AR log_q", lq, r["lq"][:Mz, :N], what, **raised(LQ_TOL, e["fl"]))


@pytest.mark.parametrize("Mp", [M_FULL, 1])
@pytest.mark.parametrize("D", [5, 21, 32])
def test_fused_ar_training(tnf, oracle, D, Mp):
    """ar_train: one forward kernel, one backward kernel (maf_bwd_mfma.hip) with ToInterval^-1 in its load stage.  The
    parameter gradient against autograd over the float64 composition: BAR_P of its largest entry, raised by 4 x the
    restatement's per-element error of the recovered point -- the relative perturbation of the stack's O(1) input."""
    c = ar_case(tnf, oracle, D)
    r = c.ref[Mp]
    p = c.params[:Mp].clone().cuda().requires_grad_()
    xin = r["xin"].cuda()
    assert c.nf._route("log_prob", xin, p) == ("ar_train", True, False)
    before = counts()
    lp = c.nf.log_prob(xin, p)
    (-(lp * c.w.cuda()).sum() / N_FULL).backward()
    assert launched(before, FORWARD_FAMILIES) == {} and launched(before, (L_.DIAG_MAF_BWD_MFMA,)) == {L_.DIAG_MAF_BWD_MFMA: 1}
    within("AR log_prob", lp, r["lp"], "ar_train D%d Mp%d" % (D, Mp), **raised(LOGP_TOL, r["e"]["il"]))
    want = c.ref_grad(Mp)
    bar = BAR_P + 4.0 * r["e"]["iz"]
    note("AR training d params", SR.gerr(p.grad, want) / bar)
    grad_err("support sweep, ar_train: d params", p.grad, want, bar)


def _coupling_nf(tnf, oracle, D, S, sup_of, seed):
    """NormFlow('coupling', support_layer=...) with small parameters and frozen statistics near the identity ->
    (nf, params, stats64, omega float64 numpy)."""
    torch.manual_seed(seed)
    nf = tnf.NormFlow(D, True, "coupling", S, 2, 15, sup_of(D))
    g = torch.Generator().manual_seed(seed)
    stats = [(torch.randn(D, generator=g) * 0.05, torch.rand(D, generator=g) * 0.1 + 0.95) for _ in nf._bn_layers()]
    for b, (m, a) in zip(nf._bn_layers(), stats):
        b.set_last_stats(m, a)
    params = torch.randn(2, nf.D_params, generator=g) * 0.05
    omega = torch.randn(2, 77, D, generator=g).clamp_(-1.8, 1.8).double().numpy()
    return nf, params, [(m.double(), a.double()) for m, a in stats], omega


CORE_FAMILIES = FORWARD_FAMILIES + (L_.DIAG_FLOW_PADDED, L_.DIAG_FLOW_PADDED_FWD)
PADDED = ("padded", {L_.DIAG_FLOW_PADDED_FWD: 1}, {L_.DIAG_FLOW_PADDED: 1})
CHAIN = ("fused", {L_.DIAG_FLOW_RANGE2_FWD: 2}, {L_.DIAG_FLOW_RANGE2: 2})  # S = 1: one launch per coupling layer


@pytest.mark.parametrize("D,fusion,expect", [(5, L_.FUSE_AUTO, PADDED), (47, L_.FUSE_AUTO, PADDED), (64, L_.FUSE_LAYER, CHAIN)],
                         ids=["padded-D5", "padded-D47", "layer-chain-D64"])
def test_unfused_interval_routes(tnf, oracle, D, fusion, expect):
    """Routes whose kernel has no support stage: ToInterval runs as its own kernel after (sampling) or before (log_prob)
    the core.  One case each pins the order of composition and the sign of the support log-det in log_prob and log_q;
    the route and the core's launches are asserted in both directions, so that neither can move to the per-bijector
    composition unnoticed."""
    family, fwd, inv = expect
    lb, ub = SR.bounds(D)
    nf, params, stats64, omega = _coupling_nf(tnf, oracle, D, 1, lambda D: tnf.ToInterval(D, lb, ub), D)
    nf.fusion = fusion
    consts = oracle.interval_consts(lb, ub)
    c7 = SR.consts7(consts)
    dims = (D, 1, 2, 15)
    with torch.no_grad(), float64():
        zc, lqc, _ = oracle.flow_forward(omega, params.double(), *dims, stats64)
        x, ldf = oracle.to_interval(zc, consts, False)
        xin = x.float()
        zi, ldi = oracle.to_interval(xin.double(), consts, True)
        lp = oracle.flow_log_prob(zi, params.double(), *dims, stats64) - ldi
    SR.assert_conditioned(xin, consts)
    fo, fl = SR.restated(zc.float(), c7, False)
    io, il = SR.restated(xin, c7, True)
    with torch.no_grad():
        for op, inp in (("log_prob", xin), ("forward", torch.tensor(omega).float())):
            assert nf._route(op, inp.cuda(), params.cuda(), True) == (family, False, False)
        before = counts()
        z, lq = nf._forward_from(omega, params.cuda(), freeze_bn=True)
        assert launched(before, CORE_FAMILIES) == fwd, launched(before, CORE_FAMILIES)
        before = counts()
        got = nf.log_prob(xin.cuda(), params.cuda())
        assert launched(before, CORE_FAMILIES) == inv, launched(before, CORE_FAMILIES)
    what = "%s D%d" % (family, D)
    within("unfused routes sampled z", z, x, what, **raised(ZF_TOL, SR.abs_err(fo, x)))
    within("unfused routes log_q", lq, lqc - ldf, what, **raised(LQ_TOL, SR.abs_err(fl, ldf)))
    within("unfused routes log_prob", got, lp, what, **raised(LOGP_TOL, SR.abs_err(il, ldi)))


@pytest.mark.parametrize("arch", ["coupling", "AR"])
def test_simplex_after_a_stack(tnf, oracle, arch):
    """ToSimplex after a coupling and an AR stack, forward only (it has no inverse): z on the simplex and log_q against the
    float64 composition; atol raised by 4 x the float32 oracle's absolute error of to_simplex on that input."""
    D = 64 if arch == "coupling" else 21
    if arch == "coupling":
        nf, params, stats64, omega = _coupling_nf(tnf, oracle, D, 1, tnf.ToSimplex, 3)
        with torch.no_grad(), float64():
            zc, lqc, _ = oracle.flow_forward(omega, params.double(), D, 1, 2, 15, stats64)
    else:
        c = ar_case(tnf, oracle, D)
        np.random.seed(1)
        torch.manual_seed(1)
        nf = tnf.NormFlow(D, True, "AR", 1, 2, 15, tnf.ToSimplex(D))
        nf.bijectors[1].set_last_stats(c.stat[0].float(), c.stat[1].float())
        params, omega = c.params, c.omega.double().numpy()
        Ms = [Mk[0].numpy() for Mk in nf.bijectors[0].Ms]
        n_maf = oracle.maf_num_params(D, 2, 15)
        with torch.no_grad(), float64():
            p64 = params.double()
            lqc = torch.tensor(oracle.base_log_density_f64(omega))
            zc, ld = oracle.maf(torch.tensor(omega), p64[:, :n_maf], D, 2, 15, Ms, False)
            lqc = lqc - ld
            zc, ld = oracle.bn_forward_frozen(zc, *c.stat)
            lqc = lqc - ld
            zc, ld = oracle.affine(zc, p64[:, n_maf:n_maf + 2 * D], D, False)
            lqc = lqc - ld
    with torch.no_grad(), float64():
        x, ldf = oracle.to_simplex(zc, D)
    with torch.no_grad():
        x32, ldf32 = oracle.to_simplex(zc.float(), D)
        z, lq = nf._forward_from(omega, params.cuda(), freeze_bn=True)
    assert z.shape[-1] == D + 1
    torch.testing.assert_close(z.sum(2).cpu(), torch.ones(z.shape[:2]), rtol=1e-5, atol=1e-5)
    what = "%s D%d" % (arch, D)
    within("ToSimplex after a stack, z", z, x, what, **raised(ZF_TOL, SR.abs_err(x32, x)))
    within("ToSimplex after a stack, log_q", lq, lqc - ldf, what, **raised(LQ_TOL, SR.abs_err(ldf32, ldf)))
