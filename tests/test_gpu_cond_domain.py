"""The fused conditioner + flow kernels (cond_flow.hip, cond_flow_bwd.hip, cond_tile.h) over their own domain: units
U from 1 to 16, every tiling TNF_OPT_COND_VARIANT compiles at every (D, H), row counts on each tiling's workgroup and
wave edges, leading dimensions and optional outputs of the C ABI, deep tile streams and degenerate upstream gradients --
in the pattern of tests/test_gpu_domain.py, section D.

Reference: the CPU oracle under float64(), on a float64 copy of param_net, float64 copies of the frozen statistics and
the same float32 x, z, omega and w, so each comparison measures the kernel's error alone.  Every fused forward asserts
exactly one cond_flow launch and no launch of another forward family.

Bars, none new: log_prob LOGP_TOL; sampled z rtol = atol = 2e-5 and log_q rtol 1e-5, atol 1e-4 (test_domain_cond_flow_
sampling); z0 and sum_log_det INV_TOL; loss rtol = atol = 1e-5 (test_domain_cond_flow_training); each gradient within
5e-5 of its largest entry, and through conftest.grad_err 1.1e-5 (d param_net) and 4e-6 (d z) as in tests/test_gpu_cond.py.
Those two tight bars are four times errors measured at U = 15, M >= 64; every case of this sweep holds them as they are
(largest measured: 2.8e-6 and 2.4e-6, both at S = 12).  When the module is done it prints the largest error per bar."""
import collections
import contextlib
import copy

import numpy as np
import pytest
import torch

from conftest import grad_err
from domain_helpers import FORWARD_FAMILIES, INV_TOL, LOGP_TOL, _cde, _net64, _stats64_of, counts, float64, launched
from torch_nf_amd import _lib as L_

pytestmark = pytest.mark.gpu

lib = L_.lib

SAMPLE_TOL = dict(rtol=2e-5, atol=2e-5)  # sampled z: test_domain_cond_flow_sampling
LOGQ_TOL = dict(rtol=1e-5, atol=1e-4)    # log_q: test_domain_cond_flow_sampling
LOSS_TOL = dict(rtol=1e-5, atol=1e-5)    # loss: test_domain_cond_flow_training
BAR_ANY, BAR_DP, BAR_DZ = 5e-5, 1.1e-5, 4e-6  # the `close` helper and the grad_err bars of tests/test_gpu_cond.py

WATCHED = FORWARD_FAMILIES + (L_.DIAG_COND_FLOW,)
ONE_COND_FLOW = {L_.DIAG_COND_FLOW: 1}

# every tiling the library compiles, per direction (launch_cond_dk, launch_bwd_dk); 0 = the automatic choice by M
VARIANTS = {"log_prob": (1, 2, 3, 4), "training": (1, 2, 3, 4, 5), "sampling": (1, 3)}
DIRECTIONS = ("log_prob", "training", "sampling")


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


@contextlib.contextmanager
def cond_variant(v):
    L_.check(lib.tnf_set_option(L_.OPT_COND_VARIANT, v))
    try:
        yield
    finally:
        L_.check(lib.tnf_set_option(L_.OPT_COND_VARIANT, 0))


_WORST = {}  # quantity -> largest observed error as a fraction of its bar, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for name, frac in sorted(_WORST.items()):
        print("largest error, %s: %.3f of the bar" % (name, frac))


def within(name, got, want, what, rtol, atol):
    """torch.testing.assert_close, after noting the largest |got - want| / (atol + rtol |want|) under `name`."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    frac = float(((got - want).abs() / (atol + rtol * want.abs())).max())
    _WORST[name] = max(frac, _WORST.get(name, 0.0))
    torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda s: "%s, %s: %s" % (name, what, s))


def close(a, b, tol=BAR_ANY):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = float(b.abs().max().clamp_min(1e-30))
    assert bool(torch.isfinite(a).all()), "non-finite gradient"
    assert float((a - b).abs().max()) <= tol * scale, (float((a - b).abs().max()), scale)


def _bare(D, S, L, H, seed, U, Dx=8):
    """param_net and frozen statistics in the _cde scheme, without the NormFlow: NormFlow, like the reference, raises
    num_units below 15 to 15, so U < 15 exists at the ops / C ABI level only -> (param_net on the device, mean, alpha)."""
    torch.manual_seed(seed)
    P = lib.tnf_flow_num_params(D, S, L, U)
    net = torch.nn.Sequential(collections.OrderedDict([("linear1", torch.nn.Linear(Dx, H)), ("tanh1", torch.nn.Tanh()),
                                                       ("linear2", torch.nn.Linear(H, P))]))
    g = torch.Generator().manual_seed(seed)
    stats = [(torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) * 0.5 + 0.75) for _ in range(2 * S)]
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.5)
    return net.cuda(), torch.stack([m for m, _ in stats]), torch.stack([a for _, a in stats])


class Case:
    """One estimator (the _cde input scheme) with fixed CPU inputs of M rows; calls take the first m rows.  The float64
    references are computed on demand, once, and never changed.  With U >= 15 the calls go through
    ConditionalDensityEstimator; below, where no NormFlow exists (_bare), through the raw entries of ops, which is where
    the module's own calls end."""

    def __init__(self, tnf, oracle, D, S, L, U, H, M, seed):
        self.tnf, self.oracle = tnf, oracle
        self.D, self.S, self.L, self.U, self.H, self.M = D, S, L, U, H, M
        self.module = U >= 15
        dev = L_.require_device()
        if self.module:
            self.nf, self.cde = _cde(tnf, D, S, L, H, seed, U=U)
            assert self.nf.num_units == U
            self.param_net = self.cde.param_net
            self.mean, self.alpha = self.nf._bn_stats(dev)
            self.stats64 = _stats64_of(self.nf)
        else:
            self.param_net, mean, alpha = _bare(D, S, L, H, seed, U)
            self.mean, self.alpha = mean.to(dev), alpha.to(dev)
            self.stats64 = [(mu.double(), al.double()) for mu, al in zip(mean, alpha)]
        g = torch.Generator().manual_seed(seed + 1)
        self.x = torch.randn(M, 8, generator=g)
        self.z = torch.randn(M, 1, D, generator=g)
        self.w = torch.rand(M, 1, generator=g) + 0.1
        self.net64 = copy.deepcopy(self.param_net).cpu().double()  # _net64
        self.dims = (D, S, L, U)
        self._ref = {}

    def __str__(self):
        return "D%d S%d L%d U%d H%d" % (self.D, self.S, self.L, self.U, self.H)

    # ---- float64 references ----
    def ref_log_prob(self):
        if "lp" not in self._ref:
            with torch.no_grad(), float64():
                lp = self.oracle.flow_log_prob(self.z.double(), self.net64(self.x.double()), *self.dims, self.stats64)
            assert lp.dtype == torch.float64
            self._ref["lp"] = lp
        return self._ref["lp"]

    def ref_sampling(self):
        """(omega float64 numpy, z, log_q) on the np.random.seed(7) draw of M rows; a draw of m < M rows is its prefix."""
        if "fwd" not in self._ref:
            np.random.seed(7)
            omega = np.random.normal(0.0, 1.0, (self.M, 1, self.D))
            with torch.no_grad(), float64():
                z, lq, _ = self.oracle.flow_forward(omega, self.net64(self.x.double()), *self.dims, self.stats64)
            assert z.dtype == lq.dtype == torch.float64
            self._ref["fwd"] = (omega, z, lq)
        return self._ref["fwd"]

    def ref_training(self, m, w=None, wkey="w"):
        """(loss, [d param_net], d z) of -(w * log_prob).mean() over the first m rows, by torch autograd over the oracle."""
        key = ("train", m, wkey)
        if key not in self._ref:
            w = self.w if w is None else w
            net = copy.deepcopy(self.net64)
            zr = self.z[:m].double().requires_grad_()
            with float64():
                lp = self.oracle.flow_log_prob(zr, net(self.x[:m].double()), *self.dims, self.stats64)
                loss = -(lp * w[:m].double()).mean()
                loss.backward()
            assert lp.dtype == torch.float64
            self._ref[key] = (loss.detach(), [p.grad for p in net.parameters()], zr.grad)
        return self._ref[key]

    # ---- the module's fused paths ----
    def log_prob(self, m, variant=0):
        zd, xd = self.z[:m].cuda(), self.x[:m].cuda()
        with cond_variant(variant), torch.no_grad():
            assert self.cde._fused_conditioner_ok(zd, xd)
            before = counts()
            lp = self.cde.log_prob(zd, xd)
            ran = launched(before, WATCHED)
        assert ran == ONE_COND_FLOW, ran
        assert lp.shape == (m, 1)
        return lp.cpu().double()

    def training(self, m, variant=0, w=None):
        w = self.w if w is None else w
        xd, wd = self.x[:m].cuda(), w[:m].cuda()
        z = self.z[:m].cuda().requires_grad_()
        self.cde.zero_grad()
        with cond_variant(variant):
            assert self.cde._fused_conditioner_ok(z, xd)
            before = counts()
            loss = -(self.cde.log_prob(z, xd) * wd).mean()
            loss.backward()
            ran = launched(before, WATCHED)
        assert ran == ONE_COND_FLOW, ran
        return loss.detach().cpu().double(), [p.grad.detach().cpu().double() for p in self.cde.param_net.parameters()], \
            z.grad.cpu().double()

    def sampling(self, m, variant=0):
        xd = self.x[:m].cuda()
        with cond_variant(variant), torch.no_grad():
            assert self.cde._fused_sampling_ok(xd)
            np.random.seed(7)
            before = counts()
            z, lq = self.cde(xd, N=1, freeze_bn=True)
            ran = launched(before, WATCHED)
        assert ran == ONE_COND_FLOW, ran
        assert z.shape == (m, 1, self.D) and lq.shape == (m, 1) and lq.dtype == torch.float64
        return z.cpu().double(), lq.cpu()

    # ---- the raw entries of ops (the module stays off them below fuse_min_contexts) ----
    def _raw_operands(self, m):
        last = self.param_net[-1]
        return self.param_net[:-1](self.x[:m].cuda()), last.weight, last.bias, self.mean, self.alpha

    def raw_log_prob(self, m, variant=0):
        with cond_variant(variant), torch.no_grad():
            before = counts()
            lp, _, _ = self.tnf.ops.cond_flow_log_prob_raw(self.z[:m, 0, :].cuda(), *self._raw_operands(m), *self.dims)
            ran = launched(before, WATCHED)
        assert ran == ONE_COND_FLOW, ran
        return lp[:, None].cpu().double()

    def raw_training(self, m, variant=0):
        z = self.z[:m, 0, :].cuda().requires_grad_()
        self.param_net.zero_grad()
        with cond_variant(variant):
            before = counts()
            lp = self.tnf.ops.cond_flow_log_prob_train(z, *self._raw_operands(m), *self.dims)
            loss = -(lp[:, None] * self.w[:m].cuda()).mean()
            loss.backward()
            ran = launched(before, WATCHED)
        assert ran == ONE_COND_FLOW, ran
        return loss.detach().cpu().double(), [p.grad.detach().cpu().double() for p in self.param_net.parameters()], \
            z.grad[:, None, :].cpu().double()

    def raw_sampling(self, m, variant=0):
        o64 = torch.from_numpy(self.ref_sampling()[0][:m]).cuda()
        with cond_variant(variant), torch.no_grad():
            before = counts()
            z, sld = self.tnf.ops.cond_flow_forward_raw(o64[:, 0, :].float(), *self._raw_operands(m), *self.dims)
            ran = launched(before, WATCHED)
            lq = self.tnf.ops.base_log_density_f64(o64) - sld[:, None]
        assert ran == ONE_COND_FLOW, ran
        return z[:, None, :].cpu().double(), lq.cpu()

    # ---- one direction at m rows under one variant, against the references ----
    def check(self, direction, section, m=None, variant=0, raw=False, w=None, wkey="w"):
        m = self.M if m is None else m
        raw = raw or not self.module
        what = "%s M%d variant %d%s" % (self, m, variant, " raw" if raw else "")
        if direction == "log_prob":
            lp = (self.raw_log_prob if raw else self.log_prob)(m, variant)
            within("log_prob", lp, self.ref_log_prob()[:m], what, **LOGP_TOL)
        elif direction == "sampling":
            z, lq = (self.raw_sampling if raw else self.sampling)(m, variant)
            _, z_r, lq_r = self.ref_sampling()
            within("sampled z", z, z_r[:m], what, **SAMPLE_TOL)
            within("log_q", lq, lq_r[:m], what, **LOGQ_TOL)
        else:
            loss, grads, gz = self.raw_training(m, variant) if raw else self.training(m, variant, w)
            loss_r, grads_r, gz_r = self.ref_training(m, w, wkey)
            within("loss", loss, loss_r, what, **LOSS_TOL)
            for a, b in zip(grads, grads_r):
                close(a, b)
                grad_err("cond sweep, %s: d param_net" % section, a, b, BAR_DP)
            close(gz, gz_r)
            grad_err("cond sweep, %s: d z" % section, gz, gz_r, BAR_DZ)


_CASES = {}


def case(tnf, oracle, D, S, L, U, H, M):
    """The Case of a shape, shared by the variants and directions that run it (same estimator, same references)."""
    key = (D, S, L, U, H, M)
    if key not in _CASES:
        _CASES[key] = Case(tnf, oracle, D, S, L, U, H, M, 1000 * S + 100 * L + 10 * U + D + H + M)
    return _CASES[key]


# ---- A. units -----------------------------------------------------------------------------------------------------
LU = [(1, 1), (1, 7), (2, 2), (2, 8), (2, 16), (3, 1), (3, 14), (5, 7)]
# H rotates over 32 / 64 / 128 along the pairs, one step further at D = 64: each (D, H) occurs two or three times
UNIT_CASES = [pytest.param(D, L, U, (32, 64, 128)[(i + D // 64) % 3], id="D%d-L%d-U%d-H%d" % (D, L, U, (32, 64, 128)[(i + D // 64) % 3]))
              for D in (32, 64) for i, (L, U) in enumerate(LU)]


@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("D,L,U,H", UNIT_CASES)
def test_units(tnf, oracle, D, L, U, H, direction):
    """Partial unit tiles: the first-layer and hidden-layer tiles carry count = U valid rows (cond_coupling_desc); the walk,
    the g_W jobs and both image kernels mask on it."""
    case(tnf, oracle, D, 2, L, U, H, 300).check(direction, "units")


def test_unit_grid_covers_every_width_twice():
    seen = [(p.values[0], p.values[3]) for p in UNIT_CASES]
    assert all(seen.count((D, H)) >= 2 for D in (32, 64) for H in (32, 64, 128))


# ---- B. tilings x widths ------------------------------------------------------------------------------------------
DH = [(D, H) for D in (32, 64) for H in (32, 64, 128)]
TILING_CASES = [pytest.param(D, H, direction, v, id="D%d-H%d-%s-variant%d" % (D, H, direction, v))
                for D, H in DH for direction in DIRECTIONS for v in VARIANTS[direction]]


@pytest.mark.parametrize("D,H,direction,variant", TILING_CASES)
def test_tilings(tnf, oracle, D, H, direction, variant):
    """M = 300 is ragged for the 64-, 128- and 256-context workgroups alike; one reference per (D, H) and direction."""
    case(tnf, oracle, D, 2, 2, 15, H, 300).check(direction, "tilings", variant=variant)


# ---- C. row edges -------------------------------------------------------------------------------------------------
ROWS = (16, 17, 33, 63, 64, 65, 129, 255, 256, 257)
RAW_ROWS = (1, 2, 15)  # below fuse_min_contexts = 16: through ops.cond_flow_*_raw / cond_flow_log_prob_train
ROW_CASES = [pytest.param(D, H, direction, v, id="D%d-H%d-%s-variant%d" % (D, H, direction, v))
             for D, H in ((64, 64), (32, 128)) for direction in DIRECTIONS for v in VARIANTS[direction]]


@pytest.mark.parametrize("D,H,direction,variant", ROW_CASES)
def test_row_edges(tnf, oracle, D, H, direction, variant):
    """Row counts around each tiling's wave (16 / 32 contexts) and workgroup (64 / 128 / 256), and around the 32-context
    groups of the g_W path: dead rows are clamped duplicates and must leave no trace.  The log_prob and sampling references
    are those of the 257 rows, sliced (the flow is row-wise); the gradient reference is per M."""
    c = case(tnf, oracle, D, 2, 2, 15, H, max(ROWS))
    assert c.cde.fuse_min_contexts == 16
    for m in RAW_ROWS:
        c.check(direction, "row edges", m, variant, raw=True)
    for m in ROWS:
        c.check(direction, "row edges", m, variant)


@pytest.mark.parametrize("M", [32768 + 77, 65536 + 77])
def test_rows_automatic_choice(tnf, oracle, M):
    """The automatic choice moves to 8 waves per workgroup at 32768 contexts and to 32 contexts per wave at 65536: the
    default variant against the float64 oracle on the first and the last 128 rows (row-wise, so the subset is exact) and
    on every row against the same call under variant 1."""
    D, S, L, U, H = 32, 1, 1, 15, 32
    nf, cde = _cde(tnf, D, S, L, H, M % 1000, U=U)
    g = torch.Generator().manual_seed(M)
    x, z = torch.randn(M, 8, generator=g), torch.randn(M, 1, D, generator=g)
    xd, zd = x.cuda(), z.cuda()
    lps = []
    for v in (0, 1):
        with cond_variant(v), torch.no_grad():
            assert cde._fused_conditioner_ok(zd, xd)
            before = counts()
            lps.append(cde.log_prob(zd, xd))
            assert launched(before, WATCHED) == ONE_COND_FLOW
    torch.testing.assert_close(lps[0], lps[1], **LOGP_TOL)
    rows = torch.cat([torch.arange(128), torch.arange(M - 128, M)])
    with torch.no_grad(), float64():
        lp_r = oracle.flow_log_prob(z[rows].double(), _net64(cde)(x[rows].double()), D, S, L, U, _stats64_of(nf))
    within("log_prob", lps[0].cpu()[rows], lp_r, "D32 S1 L1 U15 H32 M%d, first and last 128 rows" % M, **LOGP_TOL)


# ---- D. leading dimensions and optional outputs of the C ABI -------------------------------------------------------
def _bytes(n, dev):
    return torch.empty((max(1, int(n)),), dtype=torch.uint8, device=dev)


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize("H", [32, 64])
def test_abi_strides_and_optional_outputs(tnf, oracle, H):
    """tnf_cond_flow_{log_prob, forward, log_prob_fwd, log_prob_bwd}_f32 called directly (workspace and scratch sizes as
    ops.py asks for them): h and W are column slices of wider buffers whose surplus columns hold NaN (ldh = H + 4,
    ldw = H + 12), g_h and g_W slices of wider buffers (ldgh = H + 8, ldgw = H + 4).  The backward overwrites the first H
    columns of each g_h row and leaves the rest of the row alone; it zeroes all ldgw columns of every g_W row before it
    accumulates into the first H (include/tnf.h says both)."""
    D, S, L, U, M = 32, 1, 2, 15, 77
    c = case(tnf, oracle, D, S, L, U, H, M)
    dev = L_.require_device()
    nan, mark = float("nan"), 7.0
    last = c.cde.param_net[-1]
    P = last.weight.shape[0]
    assert P == lib.tnf_flow_num_params(D, S, L, U)
    mean, alpha = c.nf._bn_stats(dev)
    assert mean.is_contiguous() and alpha.is_contiguous() and mean.dtype == alpha.dtype == torch.float32
    with torch.no_grad():
        h = c.cde.param_net[:-1](c.x.cuda()).float()
        hbuf = torch.full((M, H + 4), nan, device=dev)
        hbuf[:, 4:] = h
        hs = hbuf[:, 4:]
        wbuf = torch.full((P, H + 12), nan, device=dev)
        wbuf[:, 8:8 + H] = last.weight
        Ws = wbuf[:, 8:8 + H]
        b = last.bias.detach().float().contiguous()
    ldh, ldw, ldgh, ldgw = hs.stride(0), Ws.stride(0), H + 8, H + 4
    assert (ldh, ldw) == (H + 4, H + 12)
    z = c.z[:, 0, :].contiguous().cuda()
    st = L_.stream_ptr()
    ws = _bytes(L_.check(lib.tnf_cond_flow_workspace_bytes(D, S, L, U, H)), dev)
    shape = (M, D, S, L, U, H)

    # the float64 reference on the kernel's own operands: h as the device trunk produced it, W, b, z
    last64 = copy.deepcopy(c.net64[-1])
    hr, zr = h.cpu().double().requires_grad_(), c.z.double().requires_grad_()
    with float64():
        z0_r, sld_r = oracle.flow_inverse(zr, last64(hr), D, S, L, U, c.stats64)
        lp_r = oracle.flow_log_prob(zr, last64(hr), D, S, L, U, c.stats64)
        loss_r = -(lp_r * c.w.double()).mean()
        loss_r.backward()
        omega, _, _ = c.ref_sampling()
        with torch.no_grad():
            zf_r, lq_r, _ = oracle.flow_forward(omega, last64(hr), D, S, L, U, c.stats64)

    def log_prob(want_z0, want_sld):
        lp = torch.full((M,), nan, device=dev)
        z0 = torch.full((M, D), nan, device=dev) if want_z0 else None
        sld = torch.full((M,), nan, device=dev) if want_sld else None
        before = counts()
        L_.check(lib.tnf_cond_flow_log_prob_f32(z.data_ptr(), hs.data_ptr(), Ws.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                alpha.data_ptr(), lp.data_ptr(), _p(z0), _p(sld), *shape, ldh, ldw,
                                                ws.data_ptr(), ws.numel(), st))
        assert launched(before, WATCHED) == ONE_COND_FLOW
        return lp, z0, sld

    lp, z0, sld = log_prob(True, True)
    what = "%s M%d strided" % (c, M)
    within("log_prob", lp[:, None], lp_r, what, **LOGP_TOL)
    within("z0 (C ABI)", z0[:, None, :], z0_r, what, **INV_TOL)
    within("sum_log_det (C ABI)", sld[:, None], sld_r, what, **INV_TOL)
    for want_z0, want_sld in ((False, False), (True, False), (False, True)):
        lp_o, z0_o, sld_o = log_prob(want_z0, want_sld)
        assert torch.equal(lp_o, lp), "log_prob changes with z0 %s / sum_log_det %s requested" % (want_z0, want_sld)
        assert z0_o is None or torch.equal(z0_o, z0)
        assert sld_o is None or torch.equal(sld_o, sld)

    # the sampling direction
    o64 = torch.from_numpy(omega).cuda()
    om = o64[:, 0, :].float().contiguous()
    zf, sldf = torch.full((M, D), nan, device=dev), torch.full((M,), nan, device=dev)
    before = counts()
    L_.check(lib.tnf_cond_flow_forward_f32(om.data_ptr(), hs.data_ptr(), Ws.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                           alpha.data_ptr(), zf.data_ptr(), sldf.data_ptr(), *shape, ldh, ldw,
                                           ws.data_ptr(), ws.numel(), st))
    assert launched(before, WATCHED) == ONE_COND_FLOW
    base = tnf.ops.base_log_density_f64(o64)
    within("sampled z", zf[:, None, :], zf_r, what, **SAMPLE_TOL)
    within("log_q", base - sldf[:, None], lq_r, what, **LOGQ_TOL)
    within("sum_log_det (C ABI)", sldf[:, None], base.cpu() - lq_r, what, **INV_TOL)

    # the training pair
    lpt = torch.full((M,), nan, device=dev)
    acts = torch.empty((L_.check(lib.tnf_cond_flow_acts_floats(M, D, S, L)),), dtype=torch.float32, device=dev)
    before = counts()
    L_.check(lib.tnf_cond_flow_log_prob_fwd_f32(z.data_ptr(), hs.data_ptr(), Ws.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                alpha.data_ptr(), lpt.data_ptr(), acts.data_ptr(), *shape, ldh, ldw,
                                                ws.data_ptr(), ws.numel(), st))
    assert launched(before, WATCHED) == ONE_COND_FLOW
    within("log_prob", lpt[:, None], lp_r, what, **LOGP_TOL)
    g_lp = (-c.w[:, 0] / M).cuda().contiguous()
    bws = _bytes(L_.check(lib.tnf_cond_flow_bwd_workspace_bytes(D, S, L, U, H)), dev)

    def backward(want_gz):
        deltas = torch.empty((L_.check(lib.tnf_cond_flow_deltas_floats(M, D, S, L, H)),), dtype=torch.float32, device=dev)
        ghbuf = torch.full((M, ldgh), mark, device=dev)
        ghbuf[:, 4:4 + H] = nan
        gwbuf = torch.full((P, ldgw), mark, device=dev)  # g_W at column 0: the entry zeroes P * ldgw floats from g_W on
        gwbuf[:, :H] = nan
        gb = torch.full((P,), nan, device=dev)
        gz = torch.full((M, D), nan, device=dev) if want_gz else None
        gh = ghbuf[:, 4:4 + H]
        L_.check(lib.tnf_cond_flow_log_prob_bwd_f32(g_lp.data_ptr(), hs.data_ptr(), Ws.data_ptr(), b.data_ptr(),
                                                    mean.data_ptr(), alpha.data_ptr(), acts.data_ptr(), deltas.data_ptr(),
                                                    gh.data_ptr(), gwbuf.data_ptr(), gb.data_ptr(), _p(gz), *shape, ldh, ldw,
                                                    ldgh, ldgw, bws.data_ptr(), bws.numel(), st))
        torch.cuda.synchronize()
        # surplus columns: g_h's are left alone, g_W's are zeroed
        assert bool((ghbuf[:, :4] == mark).all()) and bool((ghbuf[:, 4 + H:] == mark).all())
        assert bool((gwbuf[:, H:] == 0).all())
        return gh.clone(), gwbuf[:, :H].clone(), gb, gz

    gh, gw, gb, gz = backward(True)
    for got, want, name, bar in ((gw, last64.weight.grad, "d param_net", BAR_DP), (gb, last64.bias.grad, "d param_net", BAR_DP),
                                 (gh, hr.grad, "d h", BAR_ANY), (gz[:, None, :], zr.grad, "d z", BAR_DZ)):
        close(got, want)
        grad_err("cond sweep, C ABI: %s" % name, got, want, bar)
    gh_n, gw_n, gb_n, gz_n = backward(False)
    assert gz_n is None
    for got, want, bar in ((gh_n, gh, BAR_ANY), (gw_n, gw, BAR_DP), (gb_n, gb, BAR_DP)):
        close(got, want, bar)


# ---- E. depth -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", DIRECTIONS)
@pytest.mark.parametrize("D,S,L,U,H", [(32, 12, 2, 15, 32), (64, 8, 2, 15, 128), (64, 8, 1, 8, 64)],
                         ids=["D32-S12-L2-U15-H32", "D64-S8-L2-U15-H128", "D64-S8-L1-U8-H64"])
def test_depth(tnf, oracle, D, S, L, U, H, direction):
    """There is no cap on S: the tile stream, the saved activations and the g_W job list just get longer."""
    case(tnf, oracle, D, S, L, U, H, 300).check(direction, "depth")


# ---- F. degenerate upstream gradients -----------------------------------------------------------------------------
def test_zero_upstream_gradient(tnf, oracle):
    """w identically zero: max |g_log_prob| = 0, cond_gscale falls back to 1, and every gradient is exactly zero."""
    c = case(tnf, oracle, 32, 1, 2, 15, 32, 100)
    loss, grads, gz = c.training(100, w=torch.zeros(100, 1))
    assert float(loss) == 0.0
    for g in grads + [gz]:
        assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


def test_partly_zero_upstream_gradient(tnf, oracle):
    """w zero on the first 32-context group and on the last row: those contexts contribute nothing, the rest as usual."""
    c = case(tnf, oracle, 32, 1, 2, 15, 32, 100)
    w = c.w.clone()
    w[:32] = 0.0
    w[99] = 0.0
    c.check("training", "degenerate upstream", w=w, wkey="rows 0-31 and 99 zero")
    _, _, gz = c.training(100, w=w)
    assert bool((gz[:32] == 0).all()) and bool((gz[99] == 0).all())
