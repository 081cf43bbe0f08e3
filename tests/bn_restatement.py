"""What the Affine / BatchNorm / base-density sweep shares (tests/test_gpu_bn_domain.py on the device, tests/test_bn_host.py
without one), in the pattern of tests/maf_restatement.py: no test in here.

Float64 restatements -- the closed forms the kernels of generic_kernels.hip and backward_kernels.hip implement:
  affine64 / affine_backward64      e^a z + b, (z - b) e^-a, log_det = sum a; the gradients of backward_kernels.hip's header
  bn_apply64 / bn_apply_backward64  (z - mean) / alpha, z alpha + mean, log_det = -sum log alpha; g / alpha, g alpha
  bn_batch64                        mean = mu, alpha = sqrt(var_b + eps), z_norm = (z - mu) / alpha, log_det = -sum log alpha
  moments64                         [sum x | sum x^2 | count], every sum exact (math.fsum)
  bn_batch_backward64               dz = (1/alpha) [g - mean(g) - x^ (mean(g x^) + g_ld / n)] + g_mean / n + g_alpha x^ / n
  base64                            -1/2 sum x^2 - D/2 log 2 pi
Float32 restatements: the reference's own expressions as oracle/flow_oracle.py writes them, run on float32 tensors
(f32_*).  Their error against the float64 restatement on a case's own inputs is that case's noise; the bar of a group
(quantity, group) is 4 x the largest noise in the group -- the convention of the MAF and support sweeps.  No bar comes from
a kernel's output.

Also here: the conditioning grid and the input generators, the predicate that selects the statistics kernel and the launch
geometry of every kernel in the family, restated from the launchers, and two emulations of the statistics kernel's
accumulation -- in double, as it is, and with the float partial sums it once had (the planted fault of the host test)."""
import math

import numpy as np
import torch

from domain_helpers import float64

F64_TOL = dict(rtol=1e-9, atol=1e-9)  # tests/test_gpu_grad.py::test_affine_and_bn_grad


# ---- measures ------------------------------------------------------------------------------------------------------------
def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


def err(got, want):
    """max |got - want| / max(1, max |want|) over the case, as tests/maf_restatement.py measures values."""
    got, want = _d(got), _d(want)
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max() / max(1.0, float(want.abs().max())))


def gerr(got, want):
    """conftest.grad_err's measure: max |got - want| / max |want|."""
    got, want = _d(got), _d(want)
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


def ferr(got, want):
    """Per feature (last axis): max |got - want| / max |want| over the rows; the largest over the features.  For tensors
    whose features live on scales decades apart (alpha from 1e-3 to 1e3)."""
    got, want = _d(got), _d(want)
    D = want.shape[-1]
    diff = (got - want).abs().reshape(-1, D).max(0).values
    return float((diff / want.abs().reshape(-1, D).max(0).values.clamp_min(1e-300)).max())


class Bars:
    """noise[(quantity, group)] = the largest float32-restatement error noted for the group; bar = 4 x that."""

    def __init__(self):
        self.noise = {}

    def note(self, quantity, group, e):
        key = (quantity, group)
        self.noise[key] = max(float(e), self.noise.get(key, 0.0))

    def bar(self, quantity, group):
        return 4.0 * self.noise[(quantity, group)]

    def table(self):
        return "\n".join("  %-28s %-10s %.1e" % (q, g, v) for (q, g), v in sorted(self.noise.items(), key=str))


# ---- float64 restatements --------------------------------------------------------------------------------------------------
def affine64(z, params, D, inverse):
    z, p = _d(z), _d(params)
    a, b = p[:, None, :D], p[:, None, D:2 * D]
    out = (z - b) * torch.exp(-a) if inverse else torch.exp(a) * z + b
    return out, p[:, :D].sum(1, keepdim=True)


def affine_backward64(z, params, g_out, g_ld, D, inverse):
    """(g_z in z's shape, g_params in params' shape) for out (M, N, D), log_det (Mp, 1); a broadcast operand's gradient
    is summed over m."""
    z, p, g, gl = _d(z), _d(params), _d(g_out), _d(g_ld)
    a, b = p[:, None, :D], p[:, None, D:2 * D]
    if inverse:
        e = torch.exp(-a)
        gz, ga, gb = g * e, -(g * (z - b) * e).sum(1), -(g * e).sum(1)
    else:
        e = torch.exp(a)
        gz, ga, gb = g * e, (g * z * e).sum(1), g.sum(1)
    if z.shape[0] == 1:
        gz = gz.sum(0, keepdim=True)
    if p.shape[0] == 1:
        ga, gb = ga.sum(0, keepdim=True), gb.sum(0, keepdim=True)
    gp = torch.zeros_like(p)
    gp[:, :D] = ga + gl
    gp[:, D:2 * D] = gb
    return gz, gp


def bn_apply64(z, mean, alpha, inverse):
    z, m, a = _d(z), _d(mean), _d(alpha)
    return (z * a + m if inverse else (z - m) / a), -torch.log(a).sum()


def bn_apply_backward64(g, alpha, inverse):
    return _d(g) * _d(alpha) if inverse else _d(g) / _d(alpha)


def bn_batch64(z, eps):
    """(z_norm, log_det, mean, alpha) with the variance from centred values: no cancellation to speak of."""
    z = _d(z)
    x = z.reshape(-1, z.shape[-1])
    mu = x.mean(0)
    alpha = torch.sqrt(((x - mu) ** 2).mean(0) + eps)
    return ((x - mu) / alpha).reshape(z.shape), -torch.log(alpha).sum(), mu, alpha


def moments64(z):
    """[sum x (D) | sum x^2 (D) | rows] with exact sums, and the sums of |terms| behind the summation bound."""
    x = _d(z).reshape(-1, z.shape[-1]).numpy()
    s1 = [math.fsum(c) for c in x.T]
    s2 = [math.fsum(c * c) for c in x.T]  # the square of a float32 value is exact in double
    a1 = [math.fsum(np.abs(c)) for c in x.T]
    return np.array(s1 + s2 + [float(x.shape[0])]), np.array(a1 + s2)


def sum_bound(rows, abs_terms):
    """rows x 2^-52 of sum |term|: the worst case of a sequential double sum of exact terms (rows x 2^-53), doubled for
    the order in which the workgroups' atomics arrive."""
    return rows * 2.0 ** -52 * np.asarray(abs_terms)


def finalize64(moments, eps):
    """bn_finalize_kernel: statistics in double from the moments, rounded to float32 where the kernel stores float32.
    -> (mean, alpha, 1 / alpha, log_det)"""
    D = (len(moments) - 1) // 2
    n = moments[2 * D]
    mu = moments[:D] / n
    var = np.maximum(moments[D:2 * D] / n - mu * mu, 0.0)
    alpha = np.sqrt(var + float(np.float32(eps)))
    log_det = -np.sum(np.log(alpha.astype(np.float32)), dtype=np.float32)
    return mu.astype(np.float32), alpha.astype(np.float32), (1.0 / alpha).astype(np.float32), log_det


def kernel_model(x, eps, moments):
    """The batch-statistics forward as the kernels compute it from `moments`: bn_finalize_kernel, then
    bn_normalize_kernel's (z - mean) * (1 / alpha) in float32.  -> (z_norm, log_det, mean, alpha) as tensors."""
    mean, alpha, rstd, log_det = finalize64(moments, eps)
    zn = (np.asarray(x, dtype=np.float32) - mean) * rstd
    return tuple(torch.as_tensor(np.asarray(t)) for t in (zn, log_det, mean, alpha))


def double_moments(x):
    """[sum x | sum x^2 | rows] summed in double, in numpy's order: any order of double sums is within sum_bound."""
    x = np.asarray(x, dtype=np.float64)
    return np.concatenate([x.sum(0), (x * x).sum(0), [float(x.shape[0])]])


def bn_batch_backward64(z_norm, alpha, g_zn, g_ld, g_mean=None, g_alpha=None, count=None):
    zn, a, g = _d(z_norm), _d(alpha), _d(g_zn)
    D = zn.shape[-1]
    x, gg = zn.reshape(-1, D), g.reshape(-1, D)
    n = float(x.shape[0] if count is None else count)
    gz = (gg - gg.sum(0) / n - x * ((gg * x).sum(0) + float(g_ld)) / n) / a
    if g_mean is not None:
        gz = gz + _d(g_mean) / n
    if g_alpha is not None:
        gz = gz + x * _d(g_alpha) / n
    return gz.reshape(zn.shape)


def base64(x):
    x = _d(x)
    return -0.5 * (x * x).sum(-1) - 0.5 * x.shape[-1] * math.log(2.0 * math.pi)


# ---- float32 restatements: the oracle's expressions on float32 tensors ---------------------------------------------------------
def f32_affine(oracle, z, params, D, inverse):
    return oracle.affine(z.float(), params.float(), D, inverse)


def f32_bn_apply(oracle, z, mean, alpha, inverse):
    return (oracle.bn_inverse if inverse else oracle.bn_forward_frozen)(z.float(), mean.float(), alpha.float())


def ref_eps(eps):
    """torch's batch_norm refuses eps = 0.  1e-30 is below the double rounding of every variance of the grid (> 1e-4):
    var + 1e-30 == var, so with it the reference evaluates the expression eps = 0 stands for."""
    return eps if eps > 0.0 else 1e-30


def bn_batch_expression(z, eps):
    """oracle.bn_forward_batch with F.batch_norm spelled out in the tensor's own dtype: batch mean, biased variance,
    (z - mean) / sqrt(var + eps), then the oracle's lines for alpha and mean.  On the CPU F.batch_norm keeps the batch
    mean and variance of a float32 input in double and subtracts that mean; a kernel that RETURNS its statistics in
    float32 and normalises with what it returns (so that the cached inverse undoes the forward) cannot, and with two rows
    a hair apart the half ulp of the mean is 1e-3 of z_norm.  In float32 this is the reference's expression evaluated in
    float32; in float64 it is oracle.bn_forward_batch to rounding (tests/test_bn_host.py)."""
    D = z.shape[-1]
    z_vec = z.reshape(-1, D)
    z_norm = (z_vec - z_vec.mean(0)) / torch.sqrt(z_vec.var(0, unbiased=False) + eps)
    alpha = torch.sqrt(torch.var(z_vec, dim=0)) / torch.sqrt(torch.var(z_norm, dim=0))
    mean = torch.mean(z_vec - z_norm * alpha[None, :], dim=0)
    return z_norm.reshape(z.shape), -torch.sum(torch.log(alpha)), mean, alpha


def f32_bn_batch(z, eps):
    with torch.no_grad():
        return bn_batch_expression(z.float(), eps)


def autograd(fn, inputs, dtype):
    """Gradients of the scalar fn(*leaves) at `inputs` cast to dtype."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in inputs]
    fn(*leaves).backward()
    return [t.grad for t in leaves]


# ---- which statistics kernel, and every launch geometry -----------------------------------------------------------------------
def stats_route(D, ptr):
    return "vec" if D % 4 == 0 and D <= 1024 and ptr & 15 == 0 else "scalar"


def stats_rpi(D, route):
    """rows one workgroup reads per iteration: 256 / (D / 4) lanes per row, or 256 / min(D, 256) for the scalar kernel"""
    return 256 // (D // 4) if route == "vec" else 256 // min(D, 256)


def _ceil(a, b):
    return -(-a // b)


def stats_geometry(rows, D, route):
    """(workgroups, rows per workgroup)"""
    if route == "vec":
        blocks = max(1, min(512, _ceil(rows, 8 * stats_rpi(D, "vec"))))
    else:
        blocks = max(1, min(1024, _ceil(rows, 256)))
    return blocks, _ceil(rows, blocks)


def elementwise_blocks(total):
    return min(8192, _ceil(total, 256))


def affine_bwd_geometry(N):
    blocks = max(1, min(512, _ceil(N, 256)))
    return blocks, _ceil(N, blocks)


def base_blocks(rows):
    return min(8192, _ceil(rows * 4, 256))


GRID_STRIDE = 8192 * 256  # more elements than this and an elementwise kernel's threads take a second element


# ---- emulations of the vector statistics kernel's accumulation -----------------------------------------------------------------
def emulate_vec_moments(x, float_partials):
    """bn_stats_vec_kernel's sums of x (rows, D) float32 in its own order: per workgroup and row slot, rows r0 + r,
    + rpi, ...; in double throughout, or -- float_partials, the kernel before the sweep -- float32 sums and fused
    multiply-adds over runs of 64 rows, folded into doubles."""
    x = np.asarray(x, dtype=np.float32)
    rows, D = x.shape
    rpi = stats_rpi(D, "vec")
    blocks, rpb = stats_geometry(rows, D, "vec")
    s1, s2 = np.zeros(D), np.zeros(D)
    for b in range(blocks):
        r0, r1 = b * rpb, min(rows, (b + 1) * rpb)
        for r in range(rpi):
            mine = x[r0 + r:r1:rpi] if r0 + r < r1 else x[:0]
            b1, b2 = np.zeros(D), np.zeros(D)
            for c in range(0, len(mine), 64):
                run = mine[c:c + 64]
                if float_partials:
                    a1, a2 = np.zeros(D, np.float32), np.zeros(D, np.float32)
                    for v in run:
                        a1 = a1 + v
                        a2 = (v.astype(np.float64) * v.astype(np.float64) + a2).astype(np.float32)
                    b1, b2 = b1 + a1, b2 + a2
                else:
                    for v in run.astype(np.float64):
                        b1, b2 = b1 + v, b2 + v * v
            s1, s2 = s1 + b1, s2 + b2
    return np.concatenate([s1, s2, [float(rows)]])


# ---- the conditioning grid -------------------------------------------------------------------------------------------------
CONDS = [(0.0, 1.0), (1.0, 1.0), (10.0, 1.0), (3.0, 0.05), (10.0, 0.05), (100.0, 1.0), (100.0, 0.05)]  # (mean, sd) of a feature


def ratio(c):
    return int(round(c[0] / c[1]))


RATIOS = sorted(ratio(c) for c in CONDS)


def feature_groups(D):
    """{mean / sd: indices of the features drawn with it}: feature d has CONDS[d % 7]."""
    out = {}
    for d in range(D):
        out.setdefault(ratio(CONDS[d % len(CONDS)]), []).append(d)
    return {r: torch.tensor(i) for r, i in out.items()}


def cond_input(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.tensor([CONDS[d % len(CONDS)] for d in range(D)], dtype=torch.float64)
    return (c[:, 0] + c[:, 1] * torch.randn(rows, D, generator=g, dtype=torch.float64)).float()


FEW_ROWS = 3


def group(r, rows):
    """The group of a feature drawn with mean / sd = r in a batch of `rows` rows.  Two or three rows are groups of their
    own: their sample spread can be a small fraction of sd, which makes the float32 reference noisier by decades, and
    that noise must not widen the bars of the batches with enough rows to have the spread they were drawn with."""
    return "%d%s" % (r, "-few" if rows <= FEW_ROWS else "")


def batch_errs(got, want, D):
    """{(quantity, group): error} of (z_norm, log_det, mean, alpha) against the float64 `want`.  Per conditioning group:
    z_norm against max(1, max |z_norm|); mean against the feature's scale max(|mean|, alpha); alpha relative.  log_det is
    one number per tensor: its group is the largest ratio the tensor holds."""
    (zg, lg, mg, ag), (zw, lw, mw, aw) = [[_d(t) for t in four] for four in (got, want)]
    zg, zw = zg.reshape(-1, D), zw.reshape(-1, D)
    rows, out = zw.shape[0], {}
    for r, i in feature_groups(D).items():
        out[("z_norm", group(r, rows))] = float((zg[:, i] - zw[:, i]).abs().max() / max(1.0, float(zw[:, i].abs().max())))
        out[("mean", group(r, rows))] = float(((mg[i] - mw[i]).abs() / torch.maximum(mw[i].abs(), aw[i])).max())
        out[("alpha", group(r, rows))] = float(((ag[i] - aw[i]).abs() / aw[i]).max())
    out[("log_det", group(max(feature_groups(D)), rows))] = float((lg - lw).abs() / max(1.0, float(lw.abs())))
    return out


def grouped_gerr(got, want, D):
    """{group: gerr over the group's feature columns}: the gradient of a feature scales with 1 / alpha."""
    got, want = _d(got).reshape(-1, D), _d(want).reshape(-1, D)
    return {group(r, want.shape[0]): gerr(got[:, i], want[:, i]) for r, i in feature_groups(D).items()}


# ---- the case grid -----------------------------------------------------------------------------------------------------------
AFFINE_DS = (1, 2, 5, 63, 64, 65, 257)
LAYOUTS = ((1, 1, 1), (3, 3, 7), (3, 1, 7), (1, 4, 7), (2, 2, 300))  # (Mz, Mp, N)
STRIDE_LAYOUT = (64, 64, (1, 1, 33000))  # one grid-stride case: 2,112,000 elements
AFFINE_BWD_DS = (1, 5, 64, 255, 256, 257, 300)
AFFINE_BWD_NS = (1, 255, 256, 257)
AFFINE_BWD_LONG = (5, 131075)  # 512 workgroups of 257 rows: a short last one
BWD_LAYOUTS = ((3, 3), (3, 1), (1, 4))
APPLY_DS = (1, 5, 64, 257)
APPLY_ROWS = (1, 7, 300)
BATCH_DS = (1, 3, 4, 5, 8, 12, 60, 64, 68, 252, 256, 257, 260, 1024, 1028)
BATCH_LONG = (64, 65541)  # 512 workgroups of the vector kernel plus a tail
EPSS = (1e-5, 1e-3, 0.0)
SHARD_DS = (6, 8)  # bn_count_kernel writes the count / the vector kernel does
SHARD_ROWS = 1000
BATCH_BWD_DS = (1, 5, 64, 257, 300)
BATCH_BWD_ROWS = (2, 257)
BATCH_BWD_LONG = (5, 262151)  # the sums kernel at its 1024 workgroups, with a tail
BATCH_BWD_STRIDE = (64, 33000)  # bn_batch_bwd_apply_kernel past its grid
BASE_DS = (1, 2, 3, 4, 5, 63, 64, 65, 257)
BASE_ROWS = (1, 63, 64, 65)
BASE_LONG = (2, 524291)
FLOWS = ((64, 2, 2, 15, 2048), (32, 2, 2, 15, 2048))  # (D, S, L, U, N)
FLOW_DRAWS = 4  # base draws per shape: the float32 oracle's log_q error varies 4e-8 .. 1.4e-7 between draws of one shape


def batch_rows(D):
    """2, 3 and the row counts around one and eight iterations of a workgroup of the kernel an aligned tensor gets"""
    rpi = stats_rpi(D, stats_route(D, 0))
    return (2, 3, 8 * rpi - 1, 8 * rpi, 8 * rpi + 1, 64 * rpi + 1)


def batch_layouts(rows):
    """(M, N) with M N = rows: one context, rows / k contexts for the smallest k that divides, three contexts"""
    out = [(1, rows)]
    k = next((k for k in range(2, rows) if rows % k == 0), None)
    if k:
        out.append((rows // k, k))
    if rows % 3 == 0 and (3, rows // 3) not in out:
        out.append((3, rows // 3))
    return out


MAX_RATIO = 8192.0


def nondegenerate(x):
    """eps = 0 runs where every feature's sample |mean| / sd is at most 2^13.  The closed form the kernels implement,
    var_b = sum x^2 / n - mu^2 in double, loses (mean / sd)^2 of double's 2^-53; at 2^13 that leaves 2^-27, a quarter of a
    float32 ulp of alpha.  The grid is drawn with ratios up to 2000, so this leaves out only batches of two or three rows
    that happened to fall a hair apart -- with eps > 0 they stay, eps then bounds alpha from below."""
    x = _d(x).reshape(-1, x.shape[-1])
    return bool((x.mean(0).abs() <= MAX_RATIO * x.std(0, unbiased=False)).all())


def _randn(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Sweep:
    """The cases of each section with their float64 answers, and the bars; a section is built once, on the CPU, by the
    first test that needs it."""

    SECTIONS = ("affine", "affine_bwd", "apply", "batch", "batch_bwd", "flow")

    def __init__(self, oracle):
        self.oracle = oracle
        self.bars = Bars()
        self.built = set()

    def need(self, section):
        if section not in self.built:
            getattr(self, "_build_" + section)()
            self.built.add(section)
            print("\nnoise after section %s (bar = 4 x):\n%s" % (section, self.bars.table()))

    # a. Affine forward / inverse
    def _build_affine(self):
        self.affine = []
        shapes = [(D, lay, False) for D in AFFINE_DS for lay in LAYOUTS]
        shapes += [(STRIDE_LAYOUT[0], STRIDE_LAYOUT[2], False), (5, (3, 3, 7), True), (64, (1, 4, 7), True)]
        for D, (Mz, Mp, N), strided in shapes:
            g = torch.Generator().manual_seed(1000 * D + 10 * N + Mz + Mp)
            z = _randn(g, Mz, N, D)
            wide = torch.cat([0.5 * _randn(g, Mp, D), _randn(g, Mp, D), _randn(g, Mp, 7)], 1)
            c = Case(D=D, Mz=Mz, Mp=Mp, N=N, z=z, wide=wide, strided=strided, want={})
            for inverse in (False, True):
                c.want[inverse] = affine64(z, wide[:, :2 * D], D, inverse)
                got = f32_affine(self.oracle, z, wide[:, :2 * D], D, inverse)
                d = "inv" if inverse else "fwd"
                self.bars.note("affine z", d, err(got[0], c.want[inverse][0]))
                self.bars.note("affine ld", d, err(got[1], c.want[inverse][1]))
            self.affine.append(c)

    # b. Affine backward
    def _build_affine_bwd(self):
        self.affine_bwd = []
        shapes = [(D, N) for D in AFFINE_BWD_DS for N in AFFINE_BWD_NS] + [AFFINE_BWD_LONG]
        for D, N in shapes:
            for Mz, Mp in BWD_LAYOUTS:
                g = torch.Generator().manual_seed(7000 * D + 10 * N + Mz + Mp)
                M = max(Mz, Mp)
                z, p = _randn(g, Mz, N, D), torch.cat([0.5 * _randn(g, Mp, D), _randn(g, Mp, D)], 1)
                wz, wl = _randn(g, M, N, D), _randn(g, Mp, 1)
                c = Case(D=D, N=N, Mz=Mz, Mp=Mp, z=z, p=p, wz=wz, wl=wl, want={})
                for inverse in (False, True):
                    c.want[inverse] = affine_backward64(z, p, wz, wl, D, inverse)

                    def loss(z_, p_):
                        out, ld = self.oracle.affine(z_, p_, D, inverse)
                        return (out * wz.to(out.dtype)).sum() + (ld * wl.to(out.dtype)).sum()

                    gz, gp = autograd(loss, (z, p), torch.float32)
                    d = "inv" if inverse else "fwd"
                    self.bars.note("affine g_z", d, gerr(gz, c.want[inverse][0]))
                    self.bars.note("affine g_params", d, gerr(gp, c.want[inverse][1]))
                self.affine_bwd.append(c)

    # c. cached BatchNorm
    def _build_apply(self):
        self.apply = []
        shapes = [(D, rows) for D in APPLY_DS for rows in APPLY_ROWS] + [(STRIDE_LAYOUT[0], STRIDE_LAYOUT[2][2])]
        for D, rows in shapes:
            g = torch.Generator().manual_seed(300 * D + rows)
            z, wz, mean = _randn(g, 1, rows, D), _randn(g, 1, rows, D), _randn(g, D)
            alpha = (10.0 ** (6.0 * torch.rand(D, generator=g, dtype=torch.float64) - 3.0)).float()
            if D >= 2:
                alpha[0], alpha[-1] = 1e-3, 1e3
            c = Case(D=D, rows=rows, z=z, wz=wz, mean=mean, alpha=alpha, want={})
            for inverse in (False, True):
                out, ld = bn_apply64(z, mean, alpha, inverse)
                c.want[inverse] = (out, ld, bn_apply_backward64(wz, alpha, inverse))
                got = f32_bn_apply(self.oracle, z, mean, alpha, inverse)

                def loss(z_):
                    return (f32_bn_apply(self.oracle, z_, mean, alpha, inverse)[0] * wz).sum()

                d = "inv" if inverse else "fwd"
                self.bars.note("apply z", d, ferr(got[0], out))
                self.bars.note("apply ld", d, err(got[1], ld))
                self.bars.note("apply g_z", d, ferr(autograd(loss, (z,), torch.float32)[0], c.want[inverse][2]))
            self.apply.append(c)

    # d, e. batch statistics
    def batch_case(self, D, rows, seed=0):
        x = cond_input(rows, D, 100000 * seed + 17 * D + rows)
        c = Case(D=D, rows=rows, x=x, want={})
        for eps in EPSS if nondegenerate(x) else EPSS[:2]:
            c.want[eps] = bn_batch64(x[None], eps)
            got = f32_bn_batch(x[None], eps)
            for key, e in batch_errs(got, c.want[eps], D).items():
                self.bars.note(*key, e)
        return c

    def _build_batch(self):
        self.batch = [self.batch_case(D, rows) for D in BATCH_DS for rows in batch_rows(D)]
        self.batch.append(self.batch_case(*BATCH_LONG))
        self.shards = {D: self.batch_case(D, SHARD_ROWS, seed=1) for D in SHARD_DS}

    # f. batch-statistics backward
    def batch_bwd_case(self, D, rows, eps=1e-5, seed=0):
        x = cond_input(rows, D, 100000 * seed + 31 * D + rows)[None]
        g = torch.Generator().manual_seed(D + rows)
        w = Case(z=_randn(g, 1, rows, D), ld=3.0, mean=_randn(g, D), alpha=_randn(g, D))
        zn, _, _, alpha = bn_batch64(x, eps)
        want = bn_batch_backward64(zn, alpha, w.z, w.ld, w.mean, w.alpha)

        def loss(z_):
            zn_, ld_, mean_, alpha_ = self.oracle.bn_forward_batch(z_, eps=ref_eps(eps))
            return (zn_ * w.z).sum() + w.ld * ld_ + (mean_ * w.mean).sum() + (alpha_ * w.alpha).sum()

        for r, e in grouped_gerr(autograd(loss, (x,), torch.float32)[0], want, D).items():
            self.bars.note("batch g_z", r, e)
        return Case(D=D, rows=rows, eps=eps, x=x, w=w, want=want, loss=loss)

    def _build_batch_bwd(self):
        shapes = [(D, rows) for D in BATCH_BWD_DS for rows in BATCH_BWD_ROWS] + [BATCH_BWD_LONG, BATCH_BWD_STRIDE]
        self.batch_bwd = [self.batch_bwd_case(D, rows) for D, rows in shapes]
        self.shard_bwd = {D: self.batch_bwd_case(D, SHARD_ROWS, seed=1) for D in SHARD_DS}

    # h. carry-through: a flow whose first Affine concentrates the batch in front of the next BatchNorm
    def _build_flow(self):
        self.flows = []
        for D, S, L, U, N in FLOWS:
            g = torch.Generator().manual_seed(D)
            layout = self.oracle.flow_layout(D, S, L, U)
            params = 0.1 * _randn(g, 1, sum(n for _, n, _ in layout))
            off = 0
            for kind, n, _ in layout:
                if kind == "affine":
                    params[:, off:off + D], params[:, off + D:off + 2 * D] = -3.0, 3.0  # x -> 3 + e^-3 x: mean / sd near 60
                    break
                off += n
            for _ in range(FLOW_DRAWS):
                omega = _randn(g, 1, N, D, dtype=torch.float64).numpy()
                with float64(), torch.no_grad():
                    z64, lq64, stats64 = self.oracle.flow_forward(omega, params.double(), D, S, L, U, None)
                with torch.no_grad():
                    z32, lq32, _ = self.oracle.flow_forward(omega, params, D, S, L, U, None)
                assert z64.dtype == torch.float64 and z32.dtype == torch.float32
                self.bars.note("flow z", D, err(z32, z64))
                self.bars.note("flow log_q", D, err(lq32, lq64))
                self.flows.append(Case(D=D, S=S, L=L, U=U, N=N, params=params, omega=omega, z=z64, lq=lq64, stats=stats64))
