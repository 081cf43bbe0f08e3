"""What the MAF sweeps share (tests/test_gpu_maf_domain.py, tests/test_maf_host.py): the matrix-pipe formulation of
csrc/maf_tile.h / maf_mfma.hip / maf_bwd_mfma.hip restated in torch (differentiable, in the dtype of its inputs), the fold
of ar_fold_kernel around it, the launchers' LDS bounds and launch geometry restated, the sweep's grid, its fixed inputs
and its error measures.  A helper like tests/support_restatement.py and tests/mog_restatement.py: no test in here.

The kernels do not evaluate the nets as the oracle does: every hidden activation is carried as r = 1 / (1 + 2^a)
(h = tanh = 1 - 2 r), the factors c = 2 log2 e and -2 are folded into the weights, the column sums c * sum_k W seed the
accumulators, and alpha stays in log2 units until the log-det.  In float64 that is the oracle's function to rounding
(tests/test_maf_host.py pins it); in float32 it is the noise model of the sweep's bars."""
import math

import numpy as np
import torch

from domain_helpers import float64

LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453  # kLog2e, kLn2 of wave_prims.h
HALF_LOG_2PI = 0.91893853320467274178                # the base density's constant of maf_mfma.hip
FWD_LDS, BWD_LDS = 150 * 1024, 156 * 1024            # maf_mfma_supported, maf_bwd_mfma_supported / maf_wide_bwd_supported
M_FULL, N_FULL = 3, 65                               # rows of a forward case; every smaller layout is a slice


def err(got, want, scale=None):
    """max |got - want| / max(1, max |want|), as tests/test_gpu_mog.py measures it.  `scale`: the denominator, where
    `want` is a slice of a case whose error is measured against the whole case's largest value."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    return float((got - want).abs().max() / (max(1.0, float(want.abs().max())) if scale is None else scale))


def gerr(got, want):
    """conftest.grad_err's measure without its record: max |got - want| / max |want|."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))


# ---- the folded formulation --------------------------------------------------------------------------------------------
def _masked(params, D, L, U, Ms, pad):
    """[(W_mu M, W_alpha M)] per layer, (M_p, d_in, d_out); with `pad` zero-padded to multiples of 16 as the operand image."""
    dims = [D] + [U] * L + [D]
    out, off = [], 0
    for i in range(L + 1):
        di, do = dims[i], dims[i + 1]
        mask = torch.as_tensor(Ms[i]).to(params.dtype)[None]
        pair = []
        for _ in range(2):
            w = mask * params[:, off:off + di * do].reshape(-1, di, do)
            off += di * do
            if pad:
                w = torch.nn.functional.pad(w, (0, -do % 16, 0, -di % 16))
            pair.append(w)
        out.append(pair)
    return out


def _bmm(x, w):
    M = max(x.shape[0], w.shape[0])
    return torch.bmm(x.expand(M, -1, -1), w.expand(M, -1, -1))


def _sig2(a):
    return 1.0 / (torch.exp2(a) + 1.0)


def folded_maf(z, params, D, L, U, Ms, inverse, pad=False, drop_seed=None, half_fold=False):
    """MAF in the kernels' formulation -> (z_out (M, N, D), log_det (M, N)).  z (M_z, N, D), params (M_p, P), one of the
    M's may be 1.  `pad` runs it on the zero-padded 16-multiples the kernels use.  Two planted defects for
    tests/test_maf_host.py: `drop_seed` = l drops the column-sum seed of hidden layer l (1 .. L - 1) or, with l = L, of
    the output layer; `half_fold` folds -c instead of -2 c into the hidden and output weights (h = 1 - r).  (A stray weight
    on a wholly padded hidden unit is no defect of this formulation: the unit carries r = 1/2 and the weight enters the
    column sum, so it cancels exactly -- which is why the padded image needs no care beyond zero weights.)"""
    c = 2.0 * LOG2E
    W = _masked(params, D, L, U, Ms, pad)
    two = 1.0 if half_fold else 2.0
    w0 = [c * w for w in W[0]]
    hid = [[(c * w.sum(1, keepdim=True) * (0.0 if drop_seed == l else 1.0), (-two * c) * w) for w in W[l]] for l in range(1, L)]
    keep = 0.0 if drop_seed == L else 1.0
    out_mu = (W[L][0].sum(1, keepdim=True) * keep, -two * W[L][0])
    out_al = (LOG2E * W[L][1].sum(1, keepdim=True) * keep, (-two * LOG2E) * W[L][1])

    def nets(x):
        r = [_sig2(_bmm(x, w0[0])), _sig2(_bmm(x, w0[1]))]
        for layer in hid:
            r = [_sig2(layer[n][0] + _bmm(r[n], layer[n][1])) for n in (0, 1)]
        return out_mu[0] + _bmm(r[0], out_mu[1]), out_al[0] + _bmm(r[1], out_al[1])

    x = torch.nn.functional.pad(z, (0, -D % 16)) if pad else z
    if inverse:
        mu, al2 = nets(x)
        y = (x - mu) * torch.exp2(-al2)
    else:
        y = x
        for _ in range(D - 1):
            mu, al2 = nets(y)
            y = x * torch.exp2(al2) + mu
    return y[..., :D], LN2 * al2.sum(2)


def _ar_split(params, D, L, U):
    n = 2 * (2 * D * U + (L - 1) * U * U)
    return params[:, :n], params[:, n:n + D, None].transpose(1, 2), params[:, n + D:n + 2 * D, None].transpose(1, 2)


def folded_ar_log_prob(z, params, D, L, U, Ms, stat):
    """NormFlow('AR').log_prob as tnf_ar_flow_log_prob_f32 computes it -> (log_prob, z0, sum_log_det).  stat = (mean_bn,
    alpha_bn); parameter row [MAF | a (D) | shift (D)]; fold of ar_fold_kernel: A = alpha_bn / e^a, B = mean_bn - shift A."""
    p_maf, a, shift = _ar_split(params, D, L, U)
    mean, alpha = (s.to(params.dtype).reshape(1, 1, D) for s in stat)
    A = alpha / torch.exp(a)
    B = mean - shift * A
    z0, ld = folded_maf(z * A + B, p_maf, D, L, U, Ms, True)
    sld = ld + (a.sum(2) - torch.log(alpha).sum())
    return -0.5 * (z0 * z0).sum(2) - D * HALF_LOG_2PI - sld, z0, sld


def folded_ar_forward(omega, params, D, L, U, Ms, stat):
    """The frozen forward as tnf_ar_flow_forward_f32 computes it -> (z, sum_log_det): A = e^a / alpha_bn, B = shift - mean_bn A."""
    p_maf, a, shift = _ar_split(params, D, L, U)
    mean, alpha = (s.to(params.dtype).reshape(1, 1, D) for s in stat)
    A = torch.exp(a) / alpha
    B = shift - mean * A
    y, ld = folded_maf(omega, p_maf, D, L, U, Ms, False)
    return y * A + B, ld + (a.sum(2) - torch.log(alpha).sum())


def oracle_ar_forward(oracle, omega, params, D, L, U, Ms, stat):
    """The oracle's frozen forward composed per bijector in the dtype of its inputs -> (z, sum_log_det)."""
    n = oracle.maf_num_params(D, L, U)
    z, sld = oracle.maf(omega, params[:, :n], D, L, U, Ms, False)
    z, ld = oracle.bn_forward_frozen(z, *(s.to(params.dtype) for s in stat))
    sld = sld + ld
    z, ld = oracle.affine(z, params[:, n:n + 2 * D], D, False)
    return z, sld + ld


def oracle_ar_inverse(oracle, z, params, D, L, U, Ms, stat):
    """The oracle's inverse pass composed per bijector -> (log_prob, z0, sum_log_det)."""
    n = oracle.maf_num_params(D, L, U)
    z, sld = oracle.affine(z, params[:, n:n + 2 * D], D, True)
    z, ld = oracle.bn_inverse(z, *(s.to(params.dtype) for s in stat))
    sld = sld + ld
    z0, ld = oracle.maf(z, params[:, :n], D, L, U, Ms, True)
    sld = sld + ld
    return -0.5 * (z0 * z0).sum(2) - D * math.log(math.sqrt(2.0 * math.pi)) - sld, z0, sld


# ---- the launchers' limits and geometry, restated ------------------------------------------------------------------------
def tiles(D, U):
    return (D + 15) // 16, (U + 15) // 16


def nwg(D, L, U):
    DT, UT = tiles(D, U)
    return 2 * UT * DT + (L - 1) * 2 * UT * UT + 2 * DT * UT


def image_floats(D, L, U):
    """MafLayout::floats() = MafBLayout::fwd_floats(): the weight groups and the accumulator seeds."""
    DT, UT = tiles(D, U)
    return nwg(D, L, U) * 256 + ((L - 1) * 2 * UT + 2 * DT) * 16


def fwd_supported(D, L, U):
    """maf_mfma_supported: (11 * 16 * DT + floats()) * 4 <= 150 KB."""
    if not (1 <= D <= 64 and 1 <= L <= 5 and 1 <= U <= 64):
        return False
    return (11 * 16 * tiles(D, U)[0] + image_floats(D, L, U)) * 4 <= FWD_LDS


def bwd_smem(D, L, U, n_acc):
    """maf_bwd_smem(wl, nacc): folded image, transposed image, nacc accumulator copies, transposes' scratch, constants."""
    return (image_floats(D, L, U) + (1 + n_acc) * nwg(D, L, U) * 256 + 4 * 2 * 272 + 11 * 16 * tiles(D, U)[0] + 4) * 4


def bwd_supported(D, L, U):
    return 1 <= D <= 32 and 1 <= L <= 3 and 1 <= U <= 64 and bwd_smem(D, L, U, 1) <= BWD_LDS


def nacc(D, L, U):
    """4 private accumulator copies where they fit the LDS, else one shared copy (float atomics; fixed point when fused)."""
    return 4 if bwd_smem(D, L, U, 4) <= BWD_LDS else 1


def train_supported(D, L, U):
    return fwd_supported(D, L, U) and bwd_supported(D, L, U)


def wide_bwd_supported(D, L, U):
    """maf_wide_bwd_supported (coupling_wide_bwd.hip): the two-pass backward, taken for D = 33 .. 64 with one shared row."""
    if not (4 <= D <= 64 and D % 4 == 0 and 1 <= U <= 64 and L >= 1):
        return False
    return L <= (3 if tiles(D, U)[1] <= 2 else 2) and image_floats(D, L, U) * 4 <= BWD_LDS


def backward_route(D, L, U, Mp):
    """'mfma' (maf_bwd_mfma.hip), 'wide' (coupling_wide_bwd.hip; the same launch counter) or 'generic', float32."""
    if bwd_supported(D, L, U):
        return "mfma"
    return "wide" if Mp == 1 and wide_bwd_supported(D, L, U) else "generic"


def persistent_bx(items, per_wg, budget, M):
    return min((items + per_wg - 1) // per_wg, max(1, budget // M))


def fwd_bx(N, M):
    """grid.x of maf_mfma: one workgroup per four 16-sample tiles, at most 2048 / M per context."""
    return persistent_bx((N + 15) // 16, 4, 2048, M)


def bwd_bx(N, Mp):
    """grid.x of maf_bwd_mfma: one workgroup when it owns its context's row, else at most 512."""
    return 1 if Mp > 1 else min(((N + 15) // 16 + 3) // 4, 512)


def tiles_per_wave(N, bx):
    """The most 16-sample tiles one wave of a grid of `bx` four-wave workgroups walks."""
    return -(-((N + 15) // 16) // (4 * bx))


def adds_fbits(N, Mp):
    """launch_ar_flow_backward's fixed-point budget: terms per accumulator and the fraction bits left of 31 - 13."""
    ntiles = (N + 15) // 16
    adds = -(-ntiles // bwd_bx(N, Mp))
    fbits, v = 18, 1
    while v < adds:
        fbits, v = fbits - 1, v * 2
    return adds, max(fbits, 0)


def train_mode(D, L, U):
    """The fused backward's accumulators: 'private' (4 copies, float) or 'fixed' (one shared copy, 32-bit fixed point)."""
    return "private" if nacc(D, L, U) == 4 else "fixed"


# ---- the grid ------------------------------------------------------------------------------------------------------------
DTS = UTS = (1, 2, 3, 4)
ROWS = [(1, 1, 1), (1, 1, 15), (1, 1, 16), (1, 1, 17), (3, 3, 65), (3, 1, 33), (1, 3, 33)]
WALK_ROWS = [(512, 512, 277), (512, 1, 277)]  # 18 tiles, 2048 / 512 = 4 workgroups: two waves walk a second, ragged tile
AR_ROWS = [(1, 1, 1), (1, 1, 17), (3, 3, 65), (3, 1, 33)]
BWD_ROWS = [(1, 1, 37), (3, 3, 147), (3, 1, 37)]  # (3, 3, 147): one workgroup per row walks 10 tiles
WIDE_ROW = (2, 1, 37)
TRAIN_M, TRAIN_NS, LONG_N = 3, (37, 147), 32789  # 32,789: 2,050 tiles, the 512-workgroup cap binds, adds = 5, fbits = 15
LONG_CELLS = [(21, 2, 42), (13, 2, 31)]          # one fixed-point cell, one private-copy cell (asserted where they run)
UNSUPPORTED_FWD = [(2, 5, 4), (3, 5, 4), (4, 4, 4), (4, 5, 4)]  # (DT, L, UT)


def d_list(DT):
    """The first D of the tile count (2: the package builds no masks for D = 1), a VEC D with wholly padded q-groups, full."""
    return [2 if DT == 1 else 16 * (DT - 1) + 1, 16 * DT - 4, 16 * DT]


def u_list(UT, flow=False):
    """The first U of the tile count (MAF's minimum is 5, NormFlow's 15) and the full tile."""
    return [max(16 * (UT - 1) + 1, 15 if flow else 5), 16 * UT]


def corner_layers(DT, UT):
    """L = 3, the largest supported L and every L <= 5 the matrix-pipe kernel refuses, at the (16 DT, 16 UT) corner."""
    sup = [L for L in range(1, 6) if fwd_supported(16 * DT, L, 16 * UT)]
    return sorted({3, max(sup)} | (set(range(1, 6)) - set(sup)))


def forward_cell(DT, UT):
    """The (D, L, U) of one (DT, UT) cell of the forward sweep."""
    out = [(D, L, U) for D in d_list(DT) for U in u_list(UT) for L in (1, 2)]
    return out + [(16 * DT, L, 16 * UT) for L in corner_layers(DT, UT)]


def walk_shape(DT):
    return (d_list(DT)[0], 2, 5)


def ar_cell(DT, UT):
    """Three shapes per cell of the AR one-kernel sweep; the corner at its largest supported L."""
    (dl, dm, dh), (ul, uh) = d_list(DT), u_list(UT, flow=True)
    return [(dl, 2, uh), (dm, 1, ul), (dh, max(L for L in range(1, 6) if fwd_supported(dh, L, uh)), uh)]


def backward_cases():
    """(D, L, U) over every (DT <= 2, UT, VEC) cell and L = 1, 2, 3: U at the first unit of its tile for odd L and at the
    full tile for L = 2; the VEC D with padded q-groups for odd L, the full tile for L = 2."""
    out = []
    for DT in (1, 2):
        for UT in UTS:
            for L in (1, 2, 3):
                U = u_list(UT)[L == 2]
                out += [(d_list(DT)[0], L, U), (d_list(DT)[2 if L == 2 else 1], L, U)]
    return out


def wide_cases():
    """D = 33 .. 64, VEC only (the two-pass backward needs D % 4 == 0): one D per DT, every UT, L = 1, 2."""
    return [(D, L, u_list(UT)[L - 1]) for D in (36, 64) for UT in UTS for L in (1, 2)]


def train_cases():
    """(D, L, U) over every (DT <= 2, UT, L) cell of the fused backward; NormFlow's U >= 15."""
    out = []
    for DT in (1, 2):
        for UT in UTS:
            for L in (1, 2, 3):
                out.append((d_list(DT)[L % 3], L, u_list(UT, flow=True)[L == 2]))
    return out


def case_id(D, L, U):
    return "D%d-L%d-U%d" % (D, L, U)


# ---- the fixed inputs and their references ----------------------------------------------------------------------------------
def weight_scale(U):
    """~ 1 / sqrt(fan-in): keeps the pre-activations O(1).  z' = (z - mu) e^-alpha is ill-conditioned otherwise, and
    near-zero pre-activations put every r at 1/2, where its absolute quantisation dominates (the small-weight case)."""
    return 0.4 / math.sqrt(max(1.0, U / 16.0))


class MafCase:
    """One MAF problem: masks drawn by the package's rule (np.random.seed, then tnf.MAF), weights ~ N(0, weight_scale(U)),
    z ~ N(0, 1), float32, R rows of each.  Per direction the float64 oracle's (z, log-det), the float32 oracle's and the
    folded float32 restatement's, computed once on one batch of `blocks` * R contexts: block 0 pairs z[m] with params[m],
    block 1 z[m] with params[0], block 2 z[0] with params[m] -- every (M_z, M_p, N) of ROWS is a slice of one block."""

    def __init__(self, tnf, oracle, D, L, U, rows=(M_FULL, N_FULL), scale=None, seed=0, blocks=3, generic=True):
        self.D, self.L, self.U, self.oracle, self.blocks, self.generic = D, L, U, oracle, blocks, generic
        np.random.seed(1000 * D + 10 * U + L + seed)
        self.layer = tnf.MAF(D, L, U)
        assert (self.layer.num_layers, self.layer.num_units) == (L, U)
        self.Ms = [M[0].numpy() for M in self.layer.Ms]
        g = torch.Generator().manual_seed(7000 * D + 70 * U + L + seed)
        self.P = self.layer.count_num_params()
        self.params = torch.randn(rows[0], self.P, generator=g) * (weight_scale(U) if scale is None else scale)
        self.z = torch.randn(rows[0], rows[1], D, generator=g)
        self.rows = rows
        self._ref = {}

    def inputs(self, Mz, Mp, N):
        return self.z[:Mz, :N], self.params[:Mp]

    def ref(self, inverse):
        """{'f64', 'orc32', 'fold32'}: (z, log-det) of the whole batch."""
        if inverse not in self._ref:
            R = self.rows[0]
            own, first = list(range(R)), [0] * R
            z, p = self.z[(own + own + first)[:self.blocks * R]], self.params[(own + first + own)[:self.blocks * R]]
            args = (self.D, self.L, self.U, self.Ms, inverse)
            with torch.no_grad():
                with float64():
                    f64 = self.oracle.maf(z.double(), p.double(), *args)
                assert f64[0].dtype == torch.float64
                self._ref[inverse] = dict(f64=f64, fold32=folded_maf(z, p, *args))
                if self.generic:
                    self._ref[inverse]["orc32"] = self.oracle.maf(z, p, *args)
        return self._ref[inverse]

    def want(self, inverse, Mz, Mp, N, kind="f64"):
        block = 1 if Mp == 1 else (0 if Mz > 1 else 2)
        assert block < self.blocks
        lo = block * self.rows[0]
        z, ld = self.ref(inverse)[kind]
        return z[lo:lo + max(Mz, Mp), :N], ld[lo:lo + max(Mz, Mp), :N]

    def scale(self, inverse):
        """The case's denominators of `err` for (z, log-det): max(1, max |want|) over the whole batch -- every layout of
        the case is a slice of it and is measured against the same value, on the CPU and on the GPU."""
        return [max(1.0, float(t.abs().max())) for t in self.ref(inverse)["f64"]]

    def noise(self, inverse, kind):
        """(z, log-det) error of the float32 `kind` against float64 over the batch."""
        r = self.ref(inverse)
        return [err(r[kind][k], r["f64"][k]) for k in (0, 1)]


def maf_grads(fn, z, params, wz, wl, dtype):
    """(g_z, g_params) of sum(wz * z_out) + sum(wl * log_det) through fn(z, params) -> (z_out, log_det), in `dtype`."""
    z, params = z.detach().to(dtype, copy=True).requires_grad_(), params.detach().to(dtype, copy=True).requires_grad_()
    out, ld = fn(z, params)
    ((out * wz.to(dtype)).sum() + (ld * wl.to(dtype)).sum()).backward()
    return z.grad, params.grad


class GradCase:
    """Backward of MAF.inverse_and_log_det on one (M_z = M, M_p, N): inputs as MafCase, upstream gradients ~ N(0, 1); the
    float64 oracle's autograd gradients, the float32 oracle's and the folded float32 restatement's."""

    def __init__(self, tnf, oracle, D, L, U, M, Mp, N, scale=None):
        c = MafCase(tnf, oracle, D, L, U, rows=(M, N), scale=scale, seed=N)
        self.case, self.M, self.Mp, self.N = c, M, Mp, N
        self.z, self.params = c.z, c.params[:Mp]
        g = torch.Generator().manual_seed(N + D)
        self.wz, self.wl = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
        args = (D, L, U, c.Ms, True)
        with float64():
            self.f64 = maf_grads(lambda z, p: oracle.maf(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float64)
        assert self.f64[1].dtype == torch.float64
        self.orc32 = maf_grads(lambda z, p: oracle.maf(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float32)
        self.fold32 = maf_grads(lambda z, p: folded_maf(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float32)

    def noise(self, kind):
        got = getattr(self, kind)
        return gerr(got[0], self.f64[0]), gerr(got[1], self.f64[1])

    def masked_columns(self):
        """Indices of the parameter row whose mask entry is 0."""
        idx, off = [], 0
        for Mk in self.case.Ms:
            flat = np.concatenate([Mk.reshape(-1), Mk.reshape(-1)])
            idx += list(off + np.nonzero(flat == 0)[0])
            off += flat.size
        return idx


class ArCase:
    """NormFlow(D, True, 'AR', 1, L, U) without a support layer, frozen statistics: the MAF block as MafCase, Affine
    a ~ N(0, 0.05), shift ~ N(0, 0.1), mean_bn ~ N(0, 0.05), alpha_bn ~ U(0.95, 1.05) (the statistics of
    tests/test_gpu_support_domain.py's ArCase: the fold stays near the identity, so that the MAF sees the N(0, 1) rows the
    weight scale is chosen for), z and omega ~ N(0, 1)."""

    def __init__(self, tnf, oracle, D, L, U, rows=(M_FULL, N_FULL)):
        self.D, self.L, self.U, self.oracle, self.rows = D, L, U, oracle, rows
        np.random.seed(1000 * D + 10 * U + L)
        torch.manual_seed(D)
        self.nf = tnf.NormFlow(D, True, "AR", 1, L, U)
        assert (self.nf.num_layers, self.nf.num_units) == (L, U)
        g = torch.Generator().manual_seed(9000 * D + 90 * U + L)
        self.stat = (torch.randn(D, generator=g) * 0.05, torch.rand(D, generator=g) * 0.1 + 0.95)
        self.nf.bijectors[1].set_last_stats(*self.stat)
        self.Ms = [Mk[0].numpy() for Mk in self.nf.bijectors[0].Ms]
        self.p_maf = oracle.maf_num_params(D, L, U)
        assert self.nf.D_params == self.p_maf + 2 * D
        self.params = torch.cat((torch.randn(rows[0], self.p_maf, generator=g) * weight_scale(U),
                                 torch.randn(rows[0], D, generator=g) * 0.05, torch.randn(rows[0], D, generator=g) * 0.1), 1)
        self.z = torch.randn(rows[0], rows[1], D, generator=g)
        self._ref = {}

    def ref(self, Mp):
        """{'f64', 'fold32'}: dict(lp, z0, sld, zf, lq) on the full rows with M_p parameter rows (z = omega = self.z)."""
        if Mp not in self._ref:
            a = (self.D, self.L, self.U, self.Ms)
            out = {}
            with torch.no_grad():
                with float64():
                    st, p, z = tuple(s.double() for s in self.stat), self.params[:Mp].double(), self.z.double()
                    lp, z0, sld = oracle_ar_inverse(self.oracle, z, p, *a, st)
                    zf, sldf = oracle_ar_forward(self.oracle, z, p, *a, st)
                    base = torch.tensor(self.oracle.base_log_density_f64(z.numpy()))
                    out["f64"] = dict(lp=lp, z0=z0, sld=sld, zf=zf, lq=base - sldf)
                assert lp.dtype == zf.dtype == torch.float64
                lp, z0, sld = folded_ar_log_prob(self.z, self.params[:Mp], *a, self.stat)
                zf, sldf = folded_ar_forward(self.z, self.params[:Mp], *a, self.stat)
                out["fold32"] = dict(lp=lp, z0=z0, sld=sld, zf=zf, lq=base - sldf.double())
            self._ref[Mp] = out
        return self._ref[Mp]

    def scale(self):
        """{quantity: max(1, max |want|) over both parameter layouts}: the case's denominators of `err`."""
        return {k: max(1.0, *(float(self.ref(Mp)["f64"][k].abs().max()) for Mp in (self.rows[0], 1))) for k in self.ref(1)["f64"]}

    def noise(self):
        """{quantity: folded float32 error against float64 over both parameter layouts}."""
        sc = self.scale()
        return {k: max(err(self.ref(Mp)["fold32"][k], self.ref(Mp)["f64"][k], sc[k]) for Mp in (self.rows[0], 1)) for k in sc}


class TrainCase:
    """ar_train on (M, M_p, N): the gradient of sum(w * log_prob) w.r.t. the parameter rows, w = 10^U(-3, 0) (three
    decades, so the fixed-point scaling by the largest upstream gradient matters); float64 oracle and folded float32."""

    def __init__(self, tnf, oracle, D, L, U, M, Mp, N):
        c = ArCase(tnf, oracle, D, L, U, rows=(M, N))
        self.ar, self.M, self.Mp, self.N = c, M, Mp, N
        g = torch.Generator().manual_seed(3 * N + D)
        self.w = 10.0 ** (-3.0 * torch.rand(M, N, generator=g))
        self.params = c.params[:Mp]
        a = (D, L, U, c.Ms)
        with float64():
            p = self.params.double().requires_grad_()
            lp = oracle_ar_inverse(oracle, c.z.double(), p, *a, tuple(s.double() for s in c.stat))[0]
            (lp * self.w.double()).sum().backward()
            self.lp64, self.g64 = lp.detach(), p.grad
        assert self.g64.dtype == torch.float64
        self.g_fold32 = self._grad32(lambda z, p: folded_ar_log_prob(z, p, *a, c.stat)[0])
        self.g_orc32 = self._grad32(lambda z, p: oracle_ar_inverse(oracle, z, p, *a, c.stat)[0])

    def _grad32(self, log_prob, chunk=1024):
        """The float32 gradient, rows in chunks of 1,024 whose gradients are added in float64: the noise of the
        formulation, not of a 32,789-term float32 reduction in whatever order the host's BLAS takes it (the kernel adds
        at most two 16-sample tiles per wave before its partial sums meet)."""
        total = torch.zeros(self.params.shape, dtype=torch.float64)
        for n0 in range(0, self.N, chunk):
            p = self.params.clone().requires_grad_()
            (log_prob(self.ar.z[:, n0:n0 + chunk], p) * self.w[:, n0:n0 + chunk]).sum().backward()
            total += p.grad.double()
        return total

    def noise(self, kind="fold32"):
        return gerr(self.g_fold32 if kind == "fold32" else self.g_orc32, self.g64)


# ---- the whole sweep: every case, once per section, and the noise of each group ------------------------------------------
GENERIC_SHAPES = [(D, L, 65) for D in (65, 100) for L in (1, 2)]   # beyond the matrix-pipe domain (D, U <= 64)
GENERIC_BWD = [(33, 2, 17, 3, 3, 37), (48, 1, 64, 3, 3, 37)]      # D > 32 with per-context rows: the generic backward
SMALL_WEIGHT = (16, 3, 32, 1, 1, 147)                             # weights 0.05, L = 3: the last hidden r sits near 1/2
SMALL_SCALE = 0.05
SECTIONS = ("forward", "walk", "ar", "backward", "train")


class Sweep:
    """Every case of tests/test_gpu_maf_domain.py with its references, built once per section on first use, and `noise`:
    {(quantity, L): the largest float32 error against the float64 oracle over the group's cases} -- of the folded
    restatement for the matrix-pipe kernels (over the shapes those kernels take), of the oracle itself under
    'generic ...' (over every shape of the section)."""

    def __init__(self, tnf, oracle):
        self.tnf, self.oracle, self.noise, self.built = tnf, oracle, {}, set()

    def need(self, section):
        if section not in self.built:
            getattr(self, "_build_" + section)()
            self.built.add(section)
            print("noise, %s:\n%s" % (section, self.table(section)))
        return self

    def _directions(self, cases, prefix="", generic=True):
        for (D, L, U), c in cases:
            for inverse, name in ((True, "inverse"), (False, "sampling")):
                if fwd_supported(D, L, U):
                    self._note(prefix + name, L, c.noise(inverse, "fold32"))
                if generic:
                    self._note("generic " + name, L, c.noise(inverse, "orc32"))

    def _build_forward(self):
        self.fwd = {s: MafCase(self.tnf, self.oracle, *s) for DT in DTS for UT in UTS for s in forward_cell(DT, UT)}
        self.generic = {s: MafCase(self.tnf, self.oracle, *s) for s in GENERIC_SHAPES}
        self._directions(list(self.fwd.items()) + list(self.generic.items()))

    def _build_walk(self):
        M, _, N = WALK_ROWS[0]
        self.walk = {DT: MafCase(self.tnf, self.oracle, *walk_shape(DT), rows=(M, N), blocks=2, generic=False)
                     for DT in DTS}
        self._directions([(walk_shape(DT), c) for DT, c in self.walk.items()], "tile walk ", generic=False)

    def _build_ar(self):
        self.ar = {s: ArCase(self.tnf, self.oracle, *s) for DT in DTS for UT in UTS for s in ar_cell(DT, UT)}
        for (D, L, U), c in self.ar.items():
            for k, v in c.noise().items():
                self._add("AR " + k, L, v)

    def _build_backward(self):
        self.bwd = {}
        rows = [(s, r) for s in backward_cases() for r in BWD_ROWS] + [(s, WIDE_ROW) for s in wide_cases()]
        for (D, L, U), (M, Mp, N) in rows + [(g[:3], g[3:]) for g in GENERIC_BWD]:
            c = self.bwd[(D, L, U, M, Mp, N)] = GradCase(self.tnf, self.oracle, D, L, U, M, Mp, N)
            if backward_route(D, L, U, Mp) != "generic":
                self._note("backward", L, c.noise("fold32"), ("g_z", "g_params"))
            self._note("generic backward", L, c.noise("orc32"), ("g_z", "g_params"))
        D, L, U, M, Mp, N = SMALL_WEIGHT
        self.small = GradCase(self.tnf, self.oracle, D, L, U, M, Mp, N, scale=SMALL_SCALE)
        self._note("small-weight backward", L, self.small.noise("fold32"), ("g_z", "g_params"))
        self._note("generic backward", L, self.small.noise("orc32"), ("g_z", "g_params"))

    def _build_train(self):
        self.train = {}
        cases = [(s, TRAIN_M, Mp, N) for s in train_cases() for Mp in (TRAIN_M, 1) for N in TRAIN_NS]
        for (D, L, U), M, Mp, N in cases + [(s, 1, 1, LONG_N) for s in LONG_CELLS]:
            c = self.train[(D, L, U, M, Mp, N)] = TrainCase(self.tnf, self.oracle, D, L, U, M, Mp, N)
            if train_supported(D, L, U):
                self._add("ar_train g_params", L, c.noise())
            else:  # the per-bijector route: generic kernels (the oracle's arithmetic) and, for one shared row of a VEC D,
                   # the two-pass matrix-pipe backward (the folded arithmetic) -- the larger of the two noises
                self._add("unfused ar_train g_params", L, max(c.noise(), c.noise("orc32")))

    def _add(self, name, L, v):
        self.noise[(name, L)] = max(v, self.noise.get((name, L), 0.0))

    def _note(self, name, L, pair, parts=("z", "ld")):
        for part, v in zip(parts, pair):
            self._add("%s %s" % (name, part), L, v)

    def bar(self, name, L):
        """4 x the group's noise: room for another summation order and 1-ulp hardware exp2 / rcp, not for a lower
        precision class (the margin of conftest.grad_err's bars)."""
        return 4.0 * self.noise[(name, L)]

    def table(self, section=None):
        return "\n".join("%-34s L=%d  noise %.2e  bar %.2e" % (n, L, v, 4 * v) for (n, L), v in sorted(self.noise.items())
                         if section is None or self._section(n) == section)

    @staticmethod
    def _section(name):
        for key, sec in (("tile walk", "walk"), ("AR ", "ar"), ("ar_train", "train"), ("backward", "backward")):
            if key in name:
                return sec
        return "forward"
