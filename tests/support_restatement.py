"""What the support-layer sweeps share (tests/test_gpu_support_domain.py, tests/test_support_host.py): the fixed input
domains of ToInterval and ToSimplex, the launcher's row tiling and LDS bounds restated, the error measure, the float32
noise of the CPU oracle, and interval_fast of csrc/support_math.h restated line by line in float32 numpy.  A helper like
tests/mog_restatement.py: no test in here."""
import numpy as np
import torch

from domain_helpers import float64

KINDS = ("tanh", "lower", "upper", "identity")  # feature d of the "mixed" pattern is KINDS[d % 4]
PATTERNS = ("mixed",) + KINDS
D_LIST = (1, 2, 3, 5, 17, 31, 32, 33, 64, 127, 257, 1000, 5000)
LOG2E, LN2 = np.float32(1.4426950408889634), np.float32(0.6931471805599453)  # kLog2e, kLn2 of wave_prims.h
LDS_BUDGET, LDS_LIMIT = 32 * 1024, 64 * 1024  # rows_per_block's target and the launchers' refusal, support_kernels.hip


def err(got, want):
    """max |got - want| / max(1, max |want|), as tests/test_gpu_mog.py measures it."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


def gerr(got, want):
    """conftest.grad_err's measure without its record: max |got - want| / max |want|."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ---- the launchers' tiling (support_kernels.hip: rows_per_block and the smem checks) ----------------------------------
def rows_per_block(width, esz, planes):
    return int(min(256, max(1, LDS_BUDGET // (planes * (width + 1) * esz))))


def lds_bytes(width, esz, backward):
    """ToInterval / ToSimplex forward: R rows of width + 1; ToSimplex backward: two such planes and one value per row."""
    if backward:
        R = rows_per_block(width, esz, 3)
        return (2 * R * (width + 1) + R) * esz
    return rows_per_block(width, esz, 1) * (width + 1) * esz


def max_width(esz, backward):
    """The largest width the launcher accepts (R = 1 there): (D + 1) esz <= 64 KB, backward (2 (D + 1) + 1) esz."""
    D = (LDS_LIMIT // esz - 1) // 2 - 1 if backward else LDS_LIMIT // esz - 1
    assert lds_bytes(D, esz, backward) <= LDS_LIMIT < lds_bytes(D + 1, esz, backward)
    return D


def row_edges(R):
    """1, R - 1, R, R + 1, 2R + 1 (those that exist), ascending."""
    return sorted({r for r in (1, R - 1, R, R + 1, 2 * R + 1) if r >= 1})


# ---- the fixed input domains -----------------------------------------------------------------------------------------
def bounds(D, pattern="mixed", seed=0):
    """(lb, ub) float64: multiples of 1/8, half-widths in [0.5, 3]; a one-sided feature keeps one end of that interval."""
    rng = np.random.RandomState(1000 * seed + D)
    half = rng.randint(4, 25, D) / 8.0
    centre = rng.randint(-16, 17, D) / 8.0
    kind = np.arange(D) % 4 if pattern == "mixed" else np.full(D, KINDS.index(pattern))
    lb = np.where((kind == 0) | (kind == 1), centre - half, -np.inf)
    ub = np.where((kind == 0) | (kind == 2), centre + half, np.inf)
    return lb, ub


def consts7(consts):
    """The kernels' (7, D) float32 block from oracle.interval_consts: its six rows and the float32 log of tanh_m."""
    rows = torch.stack([c.reshape(-1) for c in consts]).float()
    return torch.cat((rows, torch.log(rows[2:3])), 0).contiguous()


def interval_draw(shape, seed):
    """z ~ N(0, 1) clamped to +-2.5, float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).clamp_(-2.5, 2.5)


def simplex_draw(shape, seed):
    """z ~ N(-1, 1), float32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) - 1.0


def assert_conditioned(x, consts):
    """x: points of the constrained space.  1 - |u| >= 0.01 on tanh features, |x - c| >= 0.05 on softplus features: a badly
    drawn case fails here rather than passing on an ill-conditioned reference."""
    tf, sf, tm, tc, _, sc = (c.reshape(-1).double() for c in consts)
    x = x.detach().double().cpu()
    u = ((x - tc) / tm)[..., tf != 0]
    s = (x - sc)[..., sf != 0]
    assert u.numel() == 0 or float(1.0 - u.abs().max()) >= 0.01, "tanh feature within 0.01 of its bound"
    assert s.numel() == 0 or float(s.abs().min()) >= 0.05, "softplus feature within 0.05 of its bound"


class IntervalCase:
    """One ToInterval problem with every reference it needs, computed once on `rows` rows (the layer is row-wise: a call
    on fewer rows compares with a slice).  z, x = the float32 oracle's forward image (the inverse's input), upstream
    gradients wz, wl; per direction the float64 oracle's (out, log_det, gradient) and the float32 oracle's."""

    def __init__(self, oracle, D, pattern, rows, seed=0):
        self.D, self.pattern, self.rows = D, pattern, rows
        self.lb, self.ub = bounds(D, pattern, seed)
        self.consts = oracle.interval_consts(self.lb, self.ub)
        self.c7 = consts7(self.consts)
        self.kind = torch.tensor([KINDS.index(pattern)] * D if pattern != "mixed" else [d % 4 for d in range(D)])
        self.z = interval_draw((1, rows, D), 7 * D + PATTERNS.index(pattern) + seed)
        with torch.no_grad():
            self.x = oracle.to_interval(self.z, self.consts, False)[0]
        assert self.x.dtype == torch.float32
        assert_conditioned(self.x, self.consts)
        g = torch.Generator().manual_seed(D + 1)
        self.wz, self.wl = torch.randn(1, rows, D, generator=g), torch.randn(1, rows, generator=g)
        self.ref64, self.ref32 = {}, {}
        for inverse in (False, True):
            inp = self.x if inverse else self.z
            with float64():
                self.ref64[inverse] = self._run(oracle, inp.double(), inverse)
            self.ref32[inverse] = self._run(oracle, inp.clone(), inverse)
            assert self.ref64[inverse][0].dtype == torch.float64 and self.ref32[inverse][0].dtype == torch.float32

    def _run(self, oracle, inp, inverse):
        inp.requires_grad_()
        out, ld = oracle.to_interval(inp, self.consts, inverse)
        ((out * self.wz.to(out.dtype)).sum() + (ld * self.wl.to(out.dtype)).sum()).backward()
        return out.detach(), ld.detach(), inp.grad

    def noise(self):
        """(values and log-dets, gradients): the float32 oracle against the float64 oracle, both directions."""
        v = max(err(self.ref32[i][k], self.ref64[i][k]) for i in (False, True) for k in (0, 1))
        g = max(gerr(self.ref32[i][2], self.ref64[i][2]) for i in (False, True))
        return v, g


class SimplexCase:
    """The same for ToSimplex: (out, log_det, gradient) of the float64 and the float32 oracle on `rows` rows."""

    def __init__(self, oracle, Din, D_attr, rows):
        self.Din, self.D_attr, self.rows = Din, D_attr, rows
        self.z = simplex_draw((1, rows, Din), 11 * Din + D_attr)
        g = torch.Generator().manual_seed(Din + 2)
        self.wz, self.wl = torch.randn(1, rows, Din + 1, generator=g), torch.randn(1, rows, generator=g)
        with float64():
            self.ref64 = self._run(oracle, self.z.double())
        self.ref32 = self._run(oracle, self.z.clone())
        assert self.ref64[0].dtype == torch.float64 and self.ref32[0].dtype == torch.float32

    def _run(self, oracle, inp):
        inp.requires_grad_()
        out, ld = oracle.to_simplex(inp, self.D_attr)
        ((out * self.wz.to(out.dtype)).sum() + (ld * self.wl.to(out.dtype)).sum()).backward()
        return out.detach(), ld.detach(), inp.grad

    def noise(self):
        return max(err(self.ref32[k], self.ref64[k]) for k in (0, 1)), gerr(self.ref32[2], self.ref64[2])


# ---- interval_fast (csrc/support_math.h) restated in float32 ----------------------------------------------------------
def _f(v):
    return np.asarray(v, dtype=np.float32)


def fast_exp(x):
    return np.exp2(LOG2E * x)  # v_exp_f32 of kLog2e x


def fast_log(x):
    return LN2 * np.log2(x)  # kLn2 v_log_f32


def fast_tanh(x):
    return _f(1) - _f(2) * (_f(1) / (np.exp2(_f(2) * LOG2E * x) + _f(1)))  # 1 - 2 sig2(kTwoLog2e x)


def fast_logsigmoid(x):
    return np.minimum(x, _f(0)) - fast_log(_f(1) + fast_exp(-np.abs(x)))


def interval_fast_restated(x, consts, inverse, flip_sign=False, permute_rows=None):
    """interval_fast<INV> on x (..., D) float32 with the (7, D) float32 constants -> (out, ld), ld per element, everything
    float32.  `flip_sign` (the sign of the tanh log-det's t * t) and `permute_rows` (a pair of constant rows to swap) plant
    one defect each: tests/test_support_host.py asserts that either pushes the error past the bar of the sweep."""
    x, c = _f(x), _f(consts).copy()
    if permute_rows is not None:
        a, b = permute_rows
        c[[a, b]] = c[[b, a]]
    tf, sf, tm, tc, sm, sc, ltm = c
    eps, one, half = _f(1e-12), _f(1), _f(0.5)
    with np.errstate(all="ignore"):
        # the tanh arm
        zi = x
        if inverse:
            u = (x - tc) * (one / tm)
            zi = half * (fast_log(one + u + eps) - fast_log(one - u + eps))
        t = fast_tanh(zi)
        t2 = t * t
        ld_t = ltm + fast_log((one + t2 if flip_sign else one - t2) + eps)
        out_t = zi if inverse else tm * t + tc
        # the softplus arm
        if inverse:
            out_s = fast_log(fast_exp((x - sc) * sm) - one + eps)
            ld_s = fast_logsigmoid(out_s)
        else:
            out_s = sm * (np.maximum(x, _f(0)) + fast_log(one + fast_exp(-np.abs(x)))) + sc
            ld_s = fast_logsigmoid(x)
    out = np.where(tf != 0, out_t, np.where(sf != 0, out_s, x))
    ld = np.where(tf != 0, ld_t, np.where(sf != 0, ld_s, _f(0)))
    assert out.dtype == ld.dtype == np.float32
    return out, ld


def restated(x, consts, inverse, **defect):
    """interval_fast_restated on a float32 tensor x (M, N, D) -> (out, log_det per row, summed in float32), tensors."""
    out, ld = interval_fast_restated(x.numpy(), consts.numpy(), inverse, **defect)
    return torch.from_numpy(out), torch.from_numpy(ld).sum(-1, dtype=torch.float32)


def abs_err(got, want):
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max())
