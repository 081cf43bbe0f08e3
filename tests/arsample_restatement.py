"""The algorithm of maf_sample_bwd_kernel (csrc/maf_sample_bwd.hip) restated in torch, dtype-generic and without
autograd: one evaluation of the twin masked MLPs at the sample, D - 1 delta-only sweeps, one last pass with the weight
gradients, and (AR-stack mode) the fold in the load stage with its three sums.  tests/test_arsample_host.py holds it to
float64 autograd through the oracle.

`folded=True` evaluates the nets the way the kernel does (build_maf_bwd_images of maf_bwd_tile.h, sections 1 .. 3 of the
kernel): every hidden activation carried as r = 1 / (1 + 2^a), c = 2 log2 e and -2 c folded into the weights, the column
sums as accumulator seeds, alpha in log2 units with e^-+alpha = exp2(-+al2); in the backward passes h = 1 - 2 r and
tanh' = 4 r (1 - r), on the plain (unfolded) transposed weights.  In float64 that is the same function (pinned by the
host tests); in float32 it is the noise model of the bars of tests/test_gpu_arsample_domain.py.

`tile=16` (one shared parameter row, M = 1) evaluates 16-row tiles as the kernel's waves do and adds the tiles' weight
gradients into a running sum of the working dtype in tile order -- an order no better than the kernel's (per-wave partial
sums, then one atomic per workgroup); torch's pairwise `sum` over 32,789 rows would understate the float32 noise."""
import torch

import maf_restatement as MR


def _weights(params, D, L, U, Ms):
    """[(W_mu, W_alpha)] per layer, masked, (M_p, in, out)."""
    return MR._masked(params, D, L, U, Ms, False)


def _evaluate(x, W, folded=False):
    """-> (inputs of every layer per net, tanh' of every hidden level per net, mu, e^-alpha, e^alpha)."""
    L = len(W) - 1
    acts, dact, outs = [[x], [x]], [[None], [None]], []
    if not folded:
        for net in range(2):
            h = x
            for i, w in enumerate(W):
                a = torch.matmul(h, w[net])
                if i < L:
                    h = torch.tanh(a)
                    acts[net].append(h)
                    dact[net].append(1.0 - h ** 2)
                else:
                    outs.append(a)
        return acts, dact, outs[0], torch.exp(-outs[1]), torch.exp(outs[1])
    c = 2.0 * MR.LOG2E
    for net in range(2):
        r = MR._sig2(torch.matmul(x, c * W[0][net]))
        for i in range(1, L + 1):
            acts[net].append(1.0 - 2.0 * r)
            dact[net].append(4.0 * r * (1.0 - r))
            outsc = c if i < L else (1.0 if net == 0 else MR.LOG2E)  # build_maf_bwd_images: outsc, wsc = -2 outsc
            a = outsc * W[i][net].sum(1, keepdim=True) + torch.matmul(r, (-2.0 * outsc) * W[i][net])
            if i < L:
                r = MR._sig2(a)
            else:
                outs.append(a)
    return acts, dact, outs[0], torch.exp2(-outs[1]), torch.exp2(outs[1])


def _back(d_mu, d_alpha, acts, dact, W, want_w):
    """Deltas back through layers L .. 0 -> (the nets' gradient w.r.t. x, [per layer (dW_mu, dW_alpha)] or None)."""
    nx, gw = 0.0, [[None, None] for _ in W]
    for net, d in ((0, d_mu), (1, d_alpha)):
        for i in range(len(W) - 1, -1, -1):
            if want_w:
                gw[i][net] = torch.matmul(acts[net][i].transpose(1, 2), d)
            d = torch.matmul(d, W[i][net].transpose(1, 2))
            if i > 0:
                d = d * dact[net][i]  # tanh' = 1 - h^2 = 4 r (1 - r)
        nx = nx + d
    return nx, (gw if want_w else None)


def _tile_ordered(g):
    """(T, in, out) per-tile gradients -> (1, in, out), added in tile order in g's dtype."""
    acc = torch.zeros_like(g[0])
    for t in range(g.shape[0]):
        acc = acc + g[t]
    return acc[None]


def maf_sample_bwd(x, params, Ms, g_x, g_ld, D, L, U, sweeps=None, folded=False, tile=None, drop_gld=False):
    """x (M, N, D) the sample, params (M_p, P), cotangents g_x (M, N, D) and g_ld (M, N)
    -> (g_omega, g_params (M_p, P), [v after each sweep]).  Two planted defects for tests/test_arsample_host.py:
    `sweeps` short of D - 1, and `drop_gld`: the - g_ld term left out of d_alpha."""
    M, N = x.shape[:2]
    if tile:  # rows as (tiles, 16, D); the pad rows carry zero cotangents, as the kernel's row_ok makes them
        assert M == 1 and params.shape[0] == 1
        pad = -N % tile
        x = torch.cat([x, x[:, -1:].expand(1, pad, D)], 1).reshape(-1, tile, D)
        g_x = torch.nn.functional.pad(g_x, (0, 0, 0, pad)).reshape(-1, tile, D)
        g_ld = torch.nn.functional.pad(g_ld, (0, pad)).reshape(-1, tile)
    W = _weights(params, D, L, U, Ms)
    acts, dact, mu, e, ea = _evaluate(x, W, folded)
    xm = x - mu

    def deltas(v):
        ve = v * e
        return -ve, -ve * xm - (0.0 if drop_gld else 1.0) * g_ld[:, :, None]

    v, trail = ea * g_x, []
    for _ in range(D - 1 if sweeps is None else sweeps):
        nv, _ = _back(*deltas(v), acts, dact, W, False)
        v = ea * (g_x - nv)
        trail.append(v)
    _, gw = _back(*deltas(v), acts, dact, W, True)
    rows = []
    for i, pair in enumerate(gw):
        mask = torch.as_tensor(Ms[i], dtype=params.dtype)[None]
        for g in pair:
            g = -(g * mask)  # g_theta = -K_theta, negated at the flush
            if tile:
                g = _tile_ordered(g)
            elif params.shape[0] == 1:
                g = g.sum(0, keepdim=True)
            rows.append(g.reshape(g.shape[0], -1))
    if tile:
        v = v.reshape(1, -1, D)[:, :N]
    return v, torch.cat(rows, 1), trail


def _fold_sum(t, Mp):
    """sum over the rows of t (M, N, K) -> (M_p, K) in the order of the kernel's fold sums (maf_sample_bwd.hip): a lane
    adds its row of every tile its wave walks, tile = 4 blockIdx.x + wave + 4 gridDim.x k (`gs_acc += gl`, `fGZ = fma(..)`,
    `fGB += g` in the load stage); the 16 sample lanes meet in an xor-shuffle tree (offsets 8, 4, 2, 1); the four waves'
    LDS rows are added in wave order (`((red[i] + red[w + i]) + red[2 * w + i]) + red[3 * w + i]`); a workgroup that does
    not own its row adds the result to global memory atomically -- here in (context, workgroup) order, one of the orders
    the atomics can take.  With pairwise `sum` instead the float32 noise of a sum that nearly cancels is understated."""
    M, N, K = t.shape
    bx = MR.bwd_bx(N, Mp)
    steps = -(-((N + 15) // 16) // (4 * bx))
    t = torch.nn.functional.pad(t, (0, 0, 0, steps * 4 * bx * 16 - N)).reshape(M, steps, 4 * bx, 16, K)
    lane = t[:, 0]
    for k in range(1, steps):
        lane = lane + t[:, k]
    for off in (8, 4, 2, 1):
        lane = lane[:, :, :off] + lane[:, :, off:]
    w = lane.reshape(M, bx, 4, K)
    wg = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    parts = [wg[m, i] for m in range(M) for i in range(bx)] if Mp == 1 else [wg[:, i] for i in range(bx)]
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total.reshape(Mp, K)


def ar_flow_sample_bwd(z, params, Ms, bn_mean, bn_alpha, g_z, g_sld, D, L, U, folded=False, drop_gs=False):
    """The AR-stack mode: z (M, N, D) the stack's output, params (M_p, P_maf + 2 D) = [MAF | a | b]
    -> g_params (M_p, P_maf + 2 D).  `folded`: the fold as ar_fold_kernel forms it (A = alpha_bn / e^a) and the three
    sums in the kernel's order (_fold_sum).  A planted defect for tests/test_arsample_host.py: `drop_gs` leaves GS out
    of g_a."""
    n = params.shape[1] - 2 * D
    a, b = params[:, n:n + D], params[:, n + D:]
    A = bn_alpha[None] / torch.exp(a) if folded else bn_alpha[None] * torch.exp(-a)
    B = bn_mean[None] - b * A
    x = z * A[:, None] + B[:, None]
    _, g_maf, _ = maf_sample_bwd(x, params[:, :n], Ms, g_z / A[:, None], g_sld, D, L, U, folded=folded)
    if folded:
        GZ, GB, GS = (_fold_sum(t, params.shape[0]) for t in (g_z * z, g_z, g_sld[:, :, None]))
        GS = GS[:, 0]
    else:
        GZ, GB, GS = (g_z * z).sum(1), g_z.sum(1), g_sld.sum(1)
    if params.shape[0] == 1 and not folded:
        GZ, GB, GS = GZ.sum(0, keepdim=True), GB.sum(0, keepdim=True), GS.sum(0, keepdim=True)
    return torch.cat([g_maf, GZ - b * GB + (0.0 if drop_gs else 1.0) * GS[:, None], GB], 1)


# ---- the sweep of tests/test_gpu_arsample_domain.py: grid, fixed inputs, references and the noise of each group ----------
# D = 1 is inside tnf_maf_sample_bwd_supported, but the package builds no masks for it (maf_masks raises), so no grid
# here has it: MR.d_list starts at D = 2.
CAP = 2e-4                                     # tests/test_gpu_arsample.py: the bound every bar but the small-weight one keeps
FLOW_ROWS = [(3, 3, 37), (3, 1, 147)]          # (c): one workgroup per row; three workgroups on the shared row
EDGE_NS = (1, 15, 16, 17)                      # (b): one row, a tile short of one row, a full tile, one row into the second
MANY_ROWS = [(130, 130, 3), (130, 1, 3)]       # (b): more contexts than one grid row of workgroups
COTANGENTS = ("both", "z", "ld")               # both cotangents, g_z (g_x) alone with the other None, g_sld (g_ld) alone
SECTIONS = ("maf", "args", "flow", "long", "small", "nf")


def vec(D):
    return D % 4 == 0


def maf_shapes():
    """(a): the supported part of MR.backward_cases()."""
    return [s for s in MR.backward_cases() if MR.bwd_supported(*s)]


def refused_shapes():
    return [s for s in MR.backward_cases() if not MR.bwd_supported(*s)]


def flow_shapes():
    """(c): the supported part of MR.train_cases()."""
    return [s for s in MR.train_cases() if MR.train_supported(*s)]


# (b): shapes of (a) -- a private-copy (nacc = 4) and a shared-copy (nacc = 1) cell, each at a VEC and at a non-VEC D
# (tests/test_arsample_host.py asserts all of that); ALIGN_CELL: D = 16, private copies
ARG_CELLS = [(16, 2, 16), (17, 1, 17), (16, 2, 48), (2, 2, 48)]
ALIGN_CELL = ARG_CELLS[0]


def arg_group(rows):
    """The noise group of a row layout of (b): one row; a tile short of a row, full, one row over; 130 contexts."""
    return "args-1row" if rows == (1, 1, 1) else "args-130" if rows in MANY_ROWS else "args-tile"


def nf_shapes():
    """(e): one shape of (c) per (DT, UT), the one with the largest L."""
    last = {}
    for s in flow_shapes():
        last[MR.tiles(s[0], s[2])] = s
    return list(last.values())


def cell(D, L, U):
    """The instantiation and run-time branch a shape takes: (DT, UT, VEC, L)."""
    return (*MR.tiles(D, U), vec(D), L)


class SampleCase:
    """tnf_maf_sample_bwd_f32 on one (M, M_p, N), every input built on the CPU: masks by the package's rule
    (np.random.seed, then tnf.MAF), weights ~ N(0, weight_scale(U)), omega ~ N(0, 1), x = float32 of the float64 oracle's
    sampling pass, cotangents ~ N(0, 1).  f64: the float64 restatement on float64 copies of those float32 inputs;
    fold32: the folded restatement in float32 (`tile`: in 16-row tiles added in tile order)."""

    def __init__(self, tnf, oracle, D, L, U, M, Mp, N, scale=None, tile=None):
        import numpy as np
        from domain_helpers import float64

        self.shape, self.rows = (D, L, U), (M, Mp, N)
        np.random.seed(1000 * D + 10 * U + L)
        self.layer = tnf.MAF(D, L, U)
        self.Ms = [Mk[0].numpy() for Mk in self.layer.Ms]
        g = torch.Generator().manual_seed(7000 * D + 70 * U + L + 13 * N + M + Mp)
        self.P = self.layer.count_num_params()
        self.params = torch.randn(Mp, self.P, generator=g) * (MR.weight_scale(U) if scale is None else scale)
        self.omega = torch.randn(M, N, D, generator=g)
        self.g_x, self.g_ld = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
        a = (D, L, U)
        with torch.no_grad():
            with float64():
                x64 = oracle.maf(self.omega.double(), self.params.double(), *a, self.Ms, False)[0]
                assert x64.dtype == torch.float64
                self.x = x64.float()
                self.f64 = maf_sample_bwd(self.x.double(), self.params.double(), self.Ms, self.g_x.double(),
                                          self.g_ld.double(), *a)[:2]
            assert self.f64[1].dtype == torch.float64
            self.fold32 = maf_sample_bwd(self.x, self.params, self.Ms, self.g_x, self.g_ld, *a, folded=True, tile=tile)[:2]
        assert self.fold32[1].dtype == torch.float32

    def noise(self):
        return MR.gerr(self.fold32[0], self.f64[0]), MR.gerr(self.fold32[1], self.f64[1])

    def masked_columns(self):
        """Indices of the parameter row whose mask entry is 0."""
        import numpy as np

        idx, off = [], 0
        for Mk in self.Ms:
            flat = np.concatenate([Mk.reshape(-1), Mk.reshape(-1)])
            idx += list(off + np.nonzero(flat == 0)[0])
            off += flat.size
        return idx


class FlowCase:
    """tnf_ar_flow_sample_bwd_f32 on one (M, M_p, N): NormFlow(D, True, 'AR', 1, L, U) for the masks, MAF block as
    SampleCase, Affine a, b ~ N(0, 0.2), frozen statistics mean ~ N(0, 0.3), alpha ~ U(0.5, 1.5), omega and the
    cotangents ~ N(0, 1); z = float32 of the float64 stack forward.  Per cotangent choice of COTANGENTS the float64
    restatement at z and the folded float32 one."""

    def __init__(self, tnf, oracle, D, L, U, M, Mp, N):
        import numpy as np
        from domain_helpers import float64

        self.shape, self.rows, self.oracle = (D, L, U), (M, Mp, N), oracle
        np.random.seed(1000 * D + 10 * U + L)
        torch.manual_seed(D)
        self.nf = tnf.NormFlow(D, True, "AR", 1, L, U)
        assert (self.nf.num_layers, self.nf.num_units) == (L, U)
        self.Ms = [Mk[0].numpy() for Mk in self.nf.bijectors[0].Ms]
        self.p_maf = oracle.maf_num_params(D, L, U)
        assert self.nf.D_params == self.p_maf + 2 * D
        g = torch.Generator().manual_seed(9000 * D + 90 * U + L + 13 * N + Mp)
        self.stat = (torch.randn(D, generator=g) * 0.3, torch.rand(D, generator=g) + 0.5)
        self.params = torch.cat((torch.randn(Mp, self.p_maf, generator=g) * MR.weight_scale(U),
                                 torch.randn(Mp, 2 * D, generator=g) * 0.2), 1)
        self.omega = torch.randn(M, N, D, generator=g)
        self.g_z, self.g_sld = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
        a = (D, L, U, self.Ms)
        self.f64, self.fold32 = {}, {}
        with torch.no_grad():
            with float64():
                st = tuple(s.double() for s in self.stat)
                z64 = MR.oracle_ar_forward(oracle, self.omega.double(), self.params.double(), *a, st)[0]
                assert z64.dtype == torch.float64
                self.z = z64.float()
                for name, gz, gs in self.cotangents():
                    self.f64[name] = ar_flow_sample_bwd(self.z.double(), self.params.double(), self.Ms, *st, gz.double(),
                                                        gs.double(), D, L, U)
            for name, gz, gs in self.cotangents():
                self.fold32[name] = ar_flow_sample_bwd(self.z, self.params, self.Ms, *self.stat, gz, gs, D, L, U, folded=True)

    def cotangents(self, none=False):
        """(name, g_z, g_sld) per COTANGENTS; `none`: None for the absent one (what the entry takes), else zeros."""
        zz, zs = (None, None) if none else (torch.zeros_like(self.g_z), torch.zeros_like(self.g_sld))
        return [("both", self.g_z, self.g_sld), ("z", self.g_z, zs), ("ld", zz, self.g_sld)]

    def split(self, g):
        return g[:, :self.p_maf], g[:, self.p_maf:]

    def noise(self):
        """(MAF block, Affine slice): the largest over the three cotangent choices."""
        pairs = [(self.split(self.fold32[k]), self.split(self.f64[k])) for k in COTANGENTS]
        return tuple(max(MR.gerr(got[i], want[i]) for got, want in pairs) for i in (0, 1))

    def nf_reference(self):
        """(e): d/d params of sum(z w_z) + sum(log_q w_l), log_q = base - sum_log_det, by float64 autograd FROM OMEGA
        through the oracle (w_z = g_z, w_l = g_sld of this case), and its noise model on the CPU: the float32 folded
        forward (MR.folded_ar_forward, what the kernel in front computes) pushed through the float32 folded backward."""
        from domain_helpers import float64

        D, L, U = self.shape
        a = (D, L, U, self.Ms)
        with float64():
            p = self.params.double().requires_grad_()
            z, sld = MR.oracle_ar_forward(self.oracle, self.omega.double(), p, *a, tuple(s.double() for s in self.stat))
            ((z * self.g_z.double()).sum() - (sld * self.g_sld.double()).sum()).backward()
        assert p.grad.dtype == torch.float64
        with torch.no_grad():
            z32 = MR.folded_ar_forward(self.omega, self.params, *a, self.stat)[0]
            fold = ar_flow_sample_bwd(z32, self.params, self.Ms, *self.stat, self.g_z, -self.g_sld, D, L, U, folded=True)
        return p.grad, fold


class Sweep:
    """Every case of tests/test_gpu_arsample_domain.py with its references, built once per section on first use, and
    `noise`: {(quantity, L): the largest error of the float32 folded restatement against float64 over the group}."""

    def __init__(self, tnf, oracle):
        self.tnf, self.oracle, self.noise, self.built = tnf, oracle, {}, set()

    def need(self, section):
        if section not in self.built:
            getattr(self, "_build_" + section)()
            self.built.add(section)
            print("noise, %s:\n%s" % (section, self.table(section)))
        return self

    def _sample(self, group, s, rows, **kw):
        c = SampleCase(self.tnf, self.oracle, *s, *rows, **kw)
        for part, v in zip(("g_omega", "g_params"), c.noise()):
            self._add("%s %s" % (group, part), s[1], v)
        return c

    def _build_maf(self):
        self.maf = {(s, r): self._sample("maf", s, r) for s in maf_shapes() for r in MR.BWD_ROWS}

    def _build_args(self):
        """The row layouts of (b), a group per kind of layout (arg_group): the gradient of a single row (N = 1) is a sum
        of one term, its float32 noise several times that of a longer sum, and must widen neither the bars of (a) nor
        those of the 130-context layouts."""
        self.args = {(s, r): self._sample(arg_group(r), s, r) for s in ARG_CELLS
                     for r in [(1, 1, N) for N in EDGE_NS] + MANY_ROWS}

    def _build_flow(self):
        self.flow = {}
        for s in flow_shapes():
            for r in FLOW_ROWS:
                c = self.flow[(s, r)] = FlowCase(self.tnf, self.oracle, *s, *r)
                for part, v in zip(("g_maf", "g_affine"), c.noise()):
                    self._add("flow " + part, s[1], v)

    def _build_long(self):
        self.long = {s: self._sample("long", s, (1, 1, MR.LONG_N), tile=16) for s in MR.LONG_CELLS}

    def _build_small(self):
        D, L, U, M, Mp, N = MR.SMALL_WEIGHT
        self.small = self._sample("small-weight", (D, L, U), (M, Mp, N), scale=MR.SMALL_SCALE)

    def _build_nf(self):
        self.need("flow")
        self.nf = {}
        for s in nf_shapes():
            c = self.flow[(s, FLOW_ROWS[0])]
            want, fold = c.nf_reference()
            self.nf[s] = (c, want)
            for part, got, ref in zip(("g_maf", "g_affine"), c.split(fold), c.split(want)):
                self._add("nf " + part, s[1], MR.gerr(got, ref))

    def _add(self, name, L, v):
        self.noise[(name, L)] = max(v, self.noise.get((name, L), 0.0))

    def bar(self, name, L):
        """4 x the group's noise: room for another summation order and 1-ulp hardware exp2 / rcp, not for a lower
        precision class (the margin of conftest.grad_err's bars and of MR.Sweep.bar).  Never above CAP, the small-weight
        group apart (tests/test_gpu_arsample_domain.py says why)."""
        bar = 4.0 * self.noise[(name, L)]
        assert bar <= CAP or name.startswith("small-weight"), (name, L, bar)
        return bar

    def table(self, section=None):
        return "\n".join("%-26s L=%d  noise %.2e  bar %.2e" % (n, L, v, 4 * v) for (n, L), v in sorted(self.noise.items())
                         if section is None or n.startswith({"small": "small-weight"}.get(section, section)))
