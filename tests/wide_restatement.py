"""What the wide RealNVP sweeps share (tests/test_gpu_wide_domain.py, tests/test_wide_host.py): the matrix-pipe formulation
of csrc/wide_tile.h (build_wide_image) + coupling_wide.hip restated in torch (differentiable, in the dtype of its inputs), the
fold that flow_fold_kernel composes around each layer of the wide per-layer chains, the launchers' LDS bounds, routes and
launch geometry restated, the sweep's grid, its fixed inputs and its error measures.  A helper like tests/maf_restatement.py:
no test in here.

The kernels do not evaluate the nets as the oracle does: every hidden activation is carried as r = 1 / (1 + 2^a)
(h = tanh = 1 - 2 r), the factors c = 2 log2 e and -2 are folded into the weights, the column sums seed the accumulators
beside the biases, and s stays in log2 units until the log-det.  In float64 that is the oracle's function to rounding
(tests/test_wide_host.py pins it); in float32 it is the noise model of the sweep's bars."""
import torch

from domain_helpers import float64
from maf_restatement import HALF_LOG_2PI, LN2, LOG2E, err, gerr, persistent_bx, weight_scale  # noqa: F401 -- err, gerr: used by the tests

FWD_LDS, BWD_LDS = 150 * 1024, 156 * 1024  # wide_supported, wide_bwd_supported
SLICES, CHUNK = 128, 1 << 18               # kWideBwdSlices, kWideBwdChunk
M_FULL, N_FULL = 3, 65                     # rows of a forward case; every smaller layout is a slice


# ---- the folded formulation --------------------------------------------------------------------------------------------
def _layers(params, D, L, U, pad):
    """[(W_t, W_s, b_t, b_s)] per MLP layer of the packed row [W_t | W_s | b_t | b_s], W (M_p, d_in, d_out), b (M_p, 1, d_out);
    with `pad` zero-padded to multiples of 16 as the operand image."""
    H = D // 2
    dims = [H] + [U] * L + [H]
    out, off = [], 0
    for i in range(L + 1):
        di, do = dims[i], dims[i + 1]
        w, b = [], []
        for _ in range(2):
            w.append(params[:, off:off + di * do].reshape(-1, di, do))
            off += di * do
        for _ in range(2):
            b.append(params[:, off:off + do].reshape(-1, 1, do))
            off += do
        if pad:
            w = [torch.nn.functional.pad(x, (0, -do % 16, 0, -di % 16)) for x in w]
            b = [torch.nn.functional.pad(x, (0, -do % 16)) for x in b]
        out.append((w[0], w[1], b[0], b[1]))
    return out


def _bmm(x, w):
    M = max(x.shape[0], w.shape[0])
    return torch.bmm(x.expand(M, -1, -1), w.expand(M, -1, -1))


def _sig2(a):
    """r = 1 / (1 + 2^a).  The clamp changes no float32 value that matters (r < 2^-126 instead of 0 where 2^a overflows,
    |a| reaches that with |x| of several hundred) and keeps autograd finite there: 0 * inf otherwise."""
    return 1.0 / (torch.exp2(a.clamp(max=126.0)) + 1.0)


def folded_coupling(z, params, D, L, U, upper, inverse, pad=False, drop_seed=None, half_fold=False):
    """One RealNVP layer in the kernels' formulation -> (z_out (M, N, D), log_det (M, N)).  z (M_z, N, D), params (M_p, P),
    one of the M's may be 1.  `pad` runs it on the zero-padded 16-multiples of H = D / 2 and U.  Planted defects for
    tests/test_wide_host.py: `drop_seed` = l drops the column-sum seed of hidden layer l (1 .. L - 1) or, with l = L, of
    the output layer; `half_fold` folds -c instead of -2 c into the weights that consume r (h = 1 - r)."""
    c, H = 2.0 * LOG2E, D // 2
    W = _layers(params, D, L, U, pad)
    two = 1.0 if half_fold else 2.0
    c_off, t_off = (0, H) if upper else (H, 0)
    x0, y = z[..., c_off:c_off + H], z[..., t_off:t_off + H]
    x = x0
    if pad:
        x, y = (torch.nn.functional.pad(v, (0, -H % 16)) for v in (x, y))
    wt, ws, bt, bs = W[0]
    r = [_sig2(c * bt + _bmm(x, c * wt)), _sig2(c * bs + _bmm(x, c * ws))]
    for l in range(1, L):
        keep = 0.0 if drop_seed == l else 1.0
        r = [_sig2(c * (b + keep * w.sum(1, keepdim=True)) + _bmm(r[n], (-two * c) * w))
             for n, (w, b) in enumerate(zip(W[l][:2], W[l][2:]))]
    wt, ws, bt, bs = W[L]
    keep = 0.0 if drop_seed == L else 1.0
    t = (bt + keep * wt.sum(1, keepdim=True)) + _bmm(r[0], -two * wt)
    s2 = LOG2E * (bs + keep * ws.sum(1, keepdim=True)) + _bmm(r[1], (-two * LOG2E) * ws)
    y = (y - t) * torch.exp2(-s2) if inverse else y * torch.exp2(s2) + t
    y = y[..., :H]
    x0 = x0.expand(y.shape[0], -1, -1)
    return torch.cat((x0, y) if upper else (y, x0), 2), LN2 * s2.sum(2)


def flow_layer_params(params, D, S, L, U, c):
    """The parameters of coupling layer c = 0 .. 2S - 1 (sampling order) inside the flow's row: per stage
    [RealNVP(upper) | RealNVP(lower) | Affine a (D) | shift (D)] (flow_layer_at)."""
    pc = 2 * (D // 2 * U * 2 + D // 2 + U + (L - 1) * (U + 1) * U)
    off = (c >> 1) * (2 * pc + 2 * D) + (c & 1) * pc
    return params[:, off:off + pc]


def fold_consts(params, D, S, L, U, stat, c, inverse):
    """fold_consts of coupling_mfma.hip for layer c -> (A, B, ld), each (M_p, 1, D) / (M_p, D): the BatchNorm behind layer c
    and, for odd c, the stage's Affine.  inverse: A = alpha / e^a, B = mean - shift A; sampling: A = e^a / alpha,
    B = shift - mean A; ld = a - log alpha."""
    mean, alpha = (s[c].to(params.dtype).reshape(1, 1, D) for s in stat)
    ld = -torch.log(alpha).reshape(1, D).expand(params.shape[0], D)
    ea, shift = torch.ones_like(alpha), torch.zeros_like(alpha)
    if c & 1:
        pc = 2 * (D // 2 * U * 2 + D // 2 + U + (L - 1) * (U + 1) * U)
        off = (c >> 1) * (2 * pc + 2 * D) + 2 * pc
        a, shift = params[:, None, off:off + D], params[:, None, off + D:off + 2 * D]
        ld, ea = ld + a[:, 0], torch.exp(a)
    if inverse:
        A = alpha / ea
        return A, mean - shift * A, ld
    A = ea / alpha
    return A, shift - mean * A, ld


def _ldc(params, D, S, L, U, stat):
    return sum(fold_consts(params, D, S, L, U, stat, c, True)[2] for c in range(2 * S)).sum(1, keepdim=True)


def folded_flow_log_prob(z, params, D, S, L, U, stat):
    """NormFlow('coupling').log_prob as the wide per-layer chain of tnf_flow_log_prob_f32 computes it (flow_fold_kernel with
    chain = 0: the fold of layer c is the `pre` stage of its kernel, on both halves) -> (log_prob, z0, sum_log_det).
    stat = (mean (2S, D), alpha (2S, D))."""
    x, sld = z, 0.0
    for c in reversed(range(2 * S)):
        A, B, _ = fold_consts(params, D, S, L, U, stat, c, True)
        x, ld = folded_coupling(x * A + B, flow_layer_params(params, D, S, L, U, c), D, L, U, c % 2 == 0, True)
        sld = sld + ld
    sld = sld + _ldc(params, D, S, L, U, stat)
    return -0.5 * (x * x).sum(2) - D * HALF_LOG_2PI - sld, x, sld


def folded_flow_forward(omega, params, D, S, L, U, stat):
    """The frozen forward as the wide chain of tnf_flow_forward_f32 computes it (the fold is the `post` stage) -> (z,
    sum_log_det)."""
    x, sld = omega, 0.0
    for c in range(2 * S):
        x, ld = folded_coupling(x, flow_layer_params(params, D, S, L, U, c), D, L, U, c % 2 == 0, False)
        A, B, _ = fold_consts(params, D, S, L, U, stat, c, False)
        x, sld = x * A + B, sld + ld
    return x, sld + _ldc(params, D, S, L, U, stat)


def stats_list(stat, dtype):
    return [(m.to(dtype), a.to(dtype)) for m, a in zip(*stat)]


# ---- the launchers' limits, routes and geometry, restated ---------------------------------------------------------------------
def tiles(D, U):
    return (D // 2 + 15) // 16, (U + 15) // 16


def layout_floats(D, L, U):
    """WideLayout::floats(): the weight groups (1 KB each) and the accumulator seeds."""
    HT, UT = tiles(D, U)
    return (4 * UT * HT + (L - 1) * 2 * UT * UT) * 256 + (2 * UT * L + 2 * HT) * 16


def wide_supported(D, L, U):
    if not (8 <= D <= 128 and D % 8 == 0 and 1 <= L <= 5 and 1 <= U <= 64):
        return False
    return (512 + layout_floats(D, L, U)) * 4 <= FWD_LDS


def bwd_layout_floats(D, L, U):
    """WideBwdLayout::floats(): the transposed raw weights of the way back."""
    HT, UT = tiles(D, U)
    return (4 * UT * HT + (L - 1) * 2 * UT * UT) * 256


def wide_bwd_supported(D, L, U):
    if not wide_supported(D, L, U) or L > (3 if tiles(D, U)[1] <= 2 else 2):
        return False
    return (layout_floats(D, L, U) + bwd_layout_floats(D, L, U)) * 4 <= BWD_LDS


def mfma_supported(D, L, U):
    return D in (32, 64) and 1 <= L <= 3 and 1 <= U <= 16


def forward_route(D, L, U, N, dtype=torch.float32, M=1, aligned=True):
    """tnf_coupling: 'narrow' (coupling_mfma.hip), 'wide' (coupling_wide.hip) or 'generic'."""
    if dtype != torch.float32 or not aligned:
        return "generic"
    if mfma_supported(D, L, U) and (N >= 16 or M >= 8):
        return "narrow"
    return "wide" if wide_supported(D, L, U) and N >= 16 else "generic"


def backward_route(D, L, U, Mp, N):
    """tnf_coupling_backward_ws, float32: the two-pass wide backward needs one shared row and has no lower bound on N."""
    if mfma_supported(D, L, U) and N >= 16:
        return "narrow"
    return "wide" if Mp == 1 and wide_bwd_supported(D, L, U) else "generic"


def fwd_bx(N, M):
    """grid.x of coupling_wide: one workgroup per four 16-sample tiles, at most 1024 / M per context."""
    return persistent_bx((N + 15) // 16, 4, 1024, M)


def bwd_bx(N):
    return persistent_bx((N + 15) // 16, 4, 512, 1)


def tiles_per_wave(N, bx):
    return -(-((N + 15) // 16) // (4 * bx))


def slicing(N):
    """Pass 2 on one chunk of N <= 2^18 samples -> (tiles per slice, non-empty slices, tiles of the last non-empty slice)."""
    assert N <= CHUNK
    ntiles = (N + 15) // 16
    per = -(-ntiles // SLICES)
    used = -(-ntiles // per)
    return per, used, ntiles - (used - 1) * per


def rec_blocks(D, L, U):
    HT, UT = tiles(D, U)
    return 3 * HT + 4 * L * UT


def num_params(D, L, U):
    return 2 * (D // 2 * U * 2 + D // 2 + U + (L - 1) * (U + 1) * U)


def bwd_workspace_bytes(N, D, L, U):
    """wide_bwd_workspace: the records of one chunk and the partial rows of every (chunk, slice)."""
    chunk = min(N, CHUNK)
    rec = (chunk + 15) // 16 * rec_blocks(D, L, U) * 256 * 4
    return -(-rec // 16) * 16 + -(-N // CHUNK) * SLICES * num_params(D, L, U) * 4


def flow_workspace_bytes(M, N, D, S, L, U, whole):
    """flow_ws of a wide shape: fold (M, 2S, 2, D) | ldc (M) | images (M, 2S, floats) [| z (M, N, D) | log-det (M, N)]."""
    def up(b):
        return -(-b // 16) * 16
    b = up(up(up(M * 2 * S * 2 * D * 4) + M * 4) + M * 2 * S * layout_floats(D, L, U) * 4)
    return b if whole else up(up(b + M * N * D * 4) + M * N * 4)


# ---- the grid ------------------------------------------------------------------------------------------------------------
HTS = UTS = (1, 2, 3, 4)
CELLS = [(HT, UT) for HT in HTS for UT in UTS]
ROWS = [(1, 1, 16), (1, 1, 17), (1, 1, 31), (3, 3, 65), (3, 1, 33), (1, 3, 33)]
GENERIC_ROWS = [(1, 1, 15), (1, 1, 1)]        # N < 16: asserted onto the generic kernel
WALK_ROWS = [(512, 512, 129), (512, 1, 129)]  # 9 tiles on 1024 / 512 = 2 workgroups: one wave walks a second, ragged tile
FLOW_ROWS = [(3, 3, 33), (3, 1, 33)]
BWD_ROWS = [(1, 1, 37), (3, 1, 37), (1, 1, 1), (3, 3, 37)]  # (3, 3, 37): per-context rows, asserted onto the generic kernel
NARROW_KEPT = (32, 2, 16)                     # the one narrow-domain shape kept, asserted onto coupling_mfma
RAW_CELL = (72, 2, 33)                        # tnf_coupling called raw: H = 36 -> 48, U = 33 -> 48
MISC_CELL = (88, 2, 17)                       # the float64 and the 4-byte-offset calls
SLICE_CELL, SLICE_NS = (8, 2, 5), (2049, 2065, 32789)
UNSUPPORTED_FWD = [(2, 5, 4), (3, 5, 4), (4, 4, 4), (4, 5, 4)]  # (HT, L, UT): no LDS for the image
LDS_REFUSED_BWD = [(3, 4, 2), (4, 4, 2)]                         # (HT, UT, L): no LDS for both images
TRAIN_SHAPES = [(24, 2, 2, 20), (72, 2, 2, 20)]                  # (D, S, L, U) of the end-to-end section, one row, N = 37


def d_list(HT):
    """The first D of the tile count, the last D with a padded q-group, the full tile (D % 8 == 0)."""
    return [32 * (HT - 1) + 8, 32 * HT - 8, 32 * HT]


def u_list(UT, flow=False):
    """The first U of the tile count (5 for UT = 1: a quarter tile; NormFlow's minimum is 15) and the full tile."""
    return [max(16 * (UT - 1) + 1, 15 if flow else 5), 16 * UT]


def corner_layers(HT, UT):
    """L = 3, the largest supported L and every L <= 5 the wide kernel refuses, at the (32 HT, 16 UT) corner."""
    sup = [L for L in range(1, 6) if wide_supported(32 * HT, L, 16 * UT)]
    return sorted({3, max(sup)} | (set(range(1, 6)) - set(sup)))


def forward_cell(HT, UT):
    """The (D, L, U) of one (HT, UT) cell of the forward sweep; a shape of the narrow domain runs L = 4, 5 instead."""
    out = []
    for D in d_list(HT):
        for U in u_list(UT):
            Ls = (1, 2) + (tuple(corner_layers(HT, UT)) if (D, U) == (32 * HT, 16 * UT) else ())
            if mfma_supported(D, 1, U):
                Ls = (4, 5)
            out += [(D, L, U) for L in sorted(set(Ls))]
    return out


def walk_shape(HT):
    return (d_list(HT)[0], 2, 5)


def flow_shapes():
    """(D, S, L, U): one padded cell per HT, UT = 2 and 4, S = 1 and 3; the L = 4 shape beyond the narrow domain and D = 128."""
    out = [(d_list(HT)[1], S, 2, u_list(UT, True)[0]) for HT in HTS for UT in (2, 4) for S in (1, 3)]
    return out + [(64, 2, 4, 15), (128, 1, 2, 32)]


def backward_shapes():
    """(D, L, U) at the padded D and U of every (HT, UT) cell: L = 1, 2, 3 (L = 3 with UT >= 3 and the two LDS-refused cells
    are routes to the generic kernel) and L = 4 at one cell."""
    out = [(d_list(HT)[1], L, u_list(UT)[0]) for HT, UT in CELLS for L in (1, 2, 3) if L < 3 or UT <= 2 or HT == 1]
    return out + [(24, 4, 17)]


def backward_direction(D, L, U):
    """(upper, inverse) pairs of a backward case: both directions, the transformed half alternating over the grid."""
    up = bool((D // 8 + L + U) % 2)
    return [(up, True), (not up, False)]


def case_id(D, L, U):
    return "D%d-L%d-U%d" % (D, L, U)


def fwd_id(D, L, U):
    HT, UT = tiles(D, U)
    return "%s-HT%d-UT%d-%s" % (case_id(D, L, U), HT, UT, forward_route(D, L, U, 16))


def bwd_id(D, L, U):
    HT, UT = tiles(D, U)
    return "%s-HT%d-UT%d-%s" % (case_id(D, L, U), HT, UT, backward_route(D, L, U, 1, 37))


# ---- the fixed inputs and their references ----------------------------------------------------------------------------------
class WideCase:
    """One RealNVP problem: weights and biases ~ N(0, weight_scale(U)), z ~ N(0, 1), float32, R rows of each.  Per (direction,
    transformed half) the float64 oracle's (z, log-det), the float32 oracle's and the folded float32 restatement's,
    computed once on one batch of `blocks` * R contexts: block 0 pairs z[m] with params[m], block 1 z[m] with params[0],
    block 2 z[0] with params[m] -- every (M_z, M_p, N) of ROWS is a slice of one block."""

    def __init__(self, oracle, D, L, U, rows=(M_FULL, N_FULL), seed=0, blocks=3, generic=True):
        self.D, self.L, self.U, self.oracle, self.blocks, self.generic, self.rows = D, L, U, oracle, blocks, generic, rows
        self.P = num_params(D, L, U)
        assert self.P == oracle.coupling_num_params(D, L, U, True) == oracle.coupling_num_params(D, L, U, False)
        for attempt in range(8):  # the first seed whose float64 references stay below 1e3 (asserted by `ref`)
            g = torch.Generator().manual_seed(7000 * D + 70 * U + L + seed + 1000003 * attempt)
            self.params = torch.randn(rows[0], self.P, generator=g) * weight_scale(U)
            self.z = torch.randn(rows[0], rows[1], D, generator=g)
            if self._largest() < 1e3:
                break
        self._ref = {}

    def _batch(self):
        R = self.rows[0]
        own, first = list(range(R)), [0] * R
        return self.z[(own + own + first)[:self.blocks * R]], self.params[(own + first + own)[:self.blocks * R]]

    def _largest(self):
        z, p = self._batch()
        with float64(), torch.no_grad():
            return max(float(self.oracle.coupling(z.double(), p.double(), self.D, self.L, self.U, up, inv)[0].abs().max())
                       for up in (True, False) for inv in (True, False))

    def inputs(self, Mz, Mp, N):
        return self.z[:Mz, :N], self.params[:Mp]

    def ref(self, inverse, upper):
        """{'f64', 'orc32', 'fold32'}: (z, log-det) of the whole batch."""
        key = (inverse, upper)
        if key not in self._ref:
            z, p = self._batch()
            args = (self.D, self.L, self.U, upper, inverse)
            with torch.no_grad():
                with float64():
                    f64 = self.oracle.coupling(z.double(), p.double(), *args)
                assert f64[0].dtype == torch.float64 and all(bool(torch.isfinite(t).all()) for t in f64)
                assert float(f64[0].abs().max()) < 1e3
                self._ref[key] = dict(f64=f64, fold32=folded_coupling(z, p, *args))
                if self.generic:
                    self._ref[key]["orc32"] = self.oracle.coupling(z, p, *args)
        return self._ref[key]

    def want(self, inverse, upper, Mz, Mp, N, kind="f64"):
        block = 1 if Mp == 1 else (0 if Mz > 1 else 2)
        assert block < self.blocks
        lo = block * self.rows[0]
        z, ld = self.ref(inverse, upper)[kind]
        return z[lo:lo + max(Mz, Mp), :N], ld[lo:lo + max(Mz, Mp), :N]

    def scale(self, inverse, upper):
        """The case's denominators of `err` for (z, log-det): max(1, max |want|) over the whole batch."""
        return [max(1.0, float(t.abs().max())) for t in self.ref(inverse, upper)["f64"]]

    def noise(self, inverse, kind):
        """(z, log-det) error of the float32 `kind` against float64 over the batch, the larger of the two halves."""
        out = [0.0, 0.0]
        for upper in (True, False):
            r = self.ref(inverse, upper)
            out = [max(o, err(r[kind][k], r["f64"][k])) for k, o in enumerate(out)]
        return out


def coupling_grads(fn, z, params, wz, wl, dtype, chunk=1024):
    """(g_z, g_params) of sum(wz * z_out) + sum(wl * log_det) through fn(z, params) -> (z_out, log_det) in `dtype`, the
    rows in chunks of 1,024 whose parameter gradients are added in float64: the noise of the formulation, not of a
    32,789-term float32 reduction in whatever order the host's BLAS takes it (pass 2 adds at most 17 tiles per slice
    before the partial rows meet in order)."""
    gz, gp = [], torch.zeros(params.shape, dtype=torch.float64)
    for n0 in range(0, z.shape[1], chunk):
        zc = z[:, n0:n0 + chunk].detach().to(dtype, copy=True).requires_grad_()
        p = params.detach().to(dtype, copy=True).requires_grad_()
        out, ld = fn(zc, p)
        ((out * wz[:, n0:n0 + chunk].to(dtype)).sum() + (ld * wl[:, n0:n0 + chunk].to(dtype)).sum()).backward()
        gz.append(zc.grad)
        gp += p.grad.double()
    return torch.cat(gz, 1), gp


class GradCase:
    """Backward of one RealNVP call on (M_z = M, M_p, N): inputs as WideCase, upstream gradients ~ N(0, 1); the float64
    oracle's autograd gradients, the float32 oracle's and the folded float32 restatement's."""

    def __init__(self, oracle, D, L, U, upper, inverse, M, Mp, N, generic=True):
        c = WideCase(oracle, D, L, U, rows=(M, N), seed=N + 2 * int(upper) + int(inverse))
        self.D, self.L, self.U, self.upper, self.inverse, self.M, self.Mp, self.N = D, L, U, upper, inverse, M, Mp, N
        self.z, self.params = c.z, c.params[:Mp]
        g = torch.Generator().manual_seed(N + D)
        self.wz, self.wl = torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)
        args = (D, L, U, upper, inverse)
        with float64():
            self.f64 = coupling_grads(lambda z, p: oracle.coupling(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float64)
        assert self.f64[1].dtype == torch.float64 and all(bool(torch.isfinite(t).all()) for t in self.f64)
        self.fold32 = coupling_grads(lambda z, p: folded_coupling(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float32)
        if generic:
            self.orc32 = coupling_grads(lambda z, p: oracle.coupling(z, p, *args), self.z, self.params, self.wz, self.wl, torch.float32)

    def noise(self, kind):
        got = getattr(self, kind)
        return gerr(got[0], self.f64[0]), gerr(got[1], self.f64[1])

    def what(self):
        return "%s %s %s (%d, %d, %d)" % (case_id(self.D, self.L, self.U), "upper" if self.upper else "lower",
                                         "inverse" if self.inverse else "forward", self.M, self.Mp, self.N)


FLOW_SEEDS = 12  # seeds tried per flow case before its weights are softened


class FlowCase:
    """NormFlow(D, True, 'coupling', S, L, U) with frozen statistics: the RealNVP blocks as WideCase, Affine a ~ N(0, 0.05),
    shift ~ N(0, 0.1), mean_bn ~ 0.1 N(0, 1), alpha_bn ~ U(0.75, 1.25) (the statistics of domain_helpers._cde), z = omega
    ~ N(0, 1): the first of FLOW_SEEDS seeds whose float64 references -- z0 and the frozen forward's z, both parameter
    layouts -- stay below 1e3.  Where no seed does (`softened`: every S = 3 cell but one), the RealNVP weights are the
    law's divided by sqrt(S).  The growth is a product of S factors e^{+-s} per feature, s being bounded by the weights
    alone (tanh), with a standard deviation of 1.3 per layer under the law: per-feature constants such as the
    statistics or the Affine cannot offset a per-sample product, and dividing by sqrt(S) gives the summed log-scale of
    a feature over its S transforms the spread the law gives one layer -- |z| and the conditioning of an S = 1 flow."""

    def __init__(self, tnf, oracle, D, S, L, U, rows=(3, 33)):
        self.D, self.S, self.L, self.U, self.oracle, self.rows = D, S, L, U, oracle, rows
        torch.manual_seed(D)
        self.nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        assert (self.nf.num_layers, self.nf.num_units) == (L, U)
        for self.softened in (False, True):
            for seed in range(FLOW_SEEDS):
                self._draw(9000 * D + 90 * U + 10 * L + S + 100000 * seed, S ** -0.5 if self.softened else 1.0)
                if all(self._largest(Mp) < 1e3 for Mp in (rows[0], 1)):
                    break
            else:
                continue
            break
        for c, b in enumerate(self.nf._bn_layers()):
            b.set_last_stats(self.stat[0][c], self.stat[1][c])

    def _largest(self, Mp):
        with float64(), torch.no_grad():
            a, p, st = (self.D, self.S, self.L, self.U), self.params[:Mp].double(), stats_list(self.stat, torch.float64)
            zf = self.oracle.flow_forward(self.z.double().numpy(), p, *a, st)[0]
            z0 = self.oracle.flow_inverse(self.z.double(), p, *a, st)[0]
        return max(float(zf.abs().max()), float(z0.abs().max()))

    def _draw(self, seed, soften):
        D, S, L, U, rows = self.D, self.S, self.L, self.U, self.rows
        g = torch.Generator().manual_seed(seed)
        pc = num_params(D, L, U)
        assert self.nf.D_params == S * (2 * pc + 2 * D) == self.oracle.flow_num_params(D, S, L, U)
        stage = [torch.cat((torch.randn(rows[0], 2 * pc, generator=g) * (weight_scale(U) * soften),
                            torch.randn(rows[0], D, generator=g) * 0.05, torch.randn(rows[0], D, generator=g) * 0.1), 1)
                 for _ in range(S)]
        self.params = torch.cat(stage, 1)
        self.stat = (torch.randn(2 * S, D, generator=g) * 0.1, torch.rand(2 * S, D, generator=g) * 0.5 + 0.75)
        self.z = torch.randn(rows[0], rows[1], D, generator=g)
        self._ref = {}

    def ref(self, Mp):
        """{'f64', 'fold32'}: dict(lp, z0, sld, zf, lq) on the full rows with M_p parameter rows (z = omega = self.z)."""
        if Mp not in self._ref:
            a = (self.D, self.S, self.L, self.U)
            out = {}
            with torch.no_grad():
                with float64():
                    st, p, z = stats_list(self.stat, torch.float64), self.params[:Mp].double(), self.z.double()
                    zf, lq, _ = self.oracle.flow_forward(z.numpy(), p, *a, st)
                    z0, sld = self.oracle.flow_inverse(z, p, *a, st)
                    lp = self.oracle.flow_log_prob(z, p, *a, st)
                    base = torch.tensor(self.oracle.base_log_density_f64(z.numpy()))
                    out["f64"] = dict(lp=lp, z0=z0, sld=sld, zf=zf, lq=lq)
                assert lp.dtype == zf.dtype == sld.dtype == torch.float64
                assert all(bool(torch.isfinite(t).all()) for t in out["f64"].values())
                assert max(float(z0.abs().max()), float(zf.abs().max())) < 1e3
                lp, z0, sld = folded_flow_log_prob(self.z, self.params[:Mp], *a, self.stat)
                zf, sldf = folded_flow_forward(self.z, self.params[:Mp], *a, self.stat)
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
    """d sum(log_prob) / d params of the flow on one shared row: the float64 oracle's autograd gradient, the folded float32
    restatement's and the float32 oracle's (the per-bijector composition runs Affine and BatchNorm kernels in the oracle's
    arithmetic around the wide coupling kernels: the bar is 4 x the larger of the two)."""

    def __init__(self, tnf, oracle, D, S, L, U, N=37):
        c = self.flow = FlowCase(tnf, oracle, D, S, L, U, rows=(1, N))
        assert not c.softened
        self.zin = c.z
        a = (D, S, L, U)

        def grad(fn, dtype):
            p = c.params.detach().to(dtype, copy=True).requires_grad_()
            fn(self.zin.to(dtype), p).sum().backward()
            return p.grad

        with float64():
            self.g64 = grad(lambda z, p: oracle.flow_log_prob(z, p, *a, stats_list(c.stat, torch.float64)), torch.float64)
        assert self.g64.dtype == torch.float64 and bool(torch.isfinite(self.g64).all())
        self.g_fold32 = grad(lambda z, p: folded_flow_log_prob(z, p, *a, c.stat)[0], torch.float32)
        self.g_orc32 = grad(lambda z, p: oracle.flow_log_prob(z, p, *a, stats_list(c.stat, torch.float32)), torch.float32)

    def noise(self):
        return max(gerr(self.g_fold32, self.g64), gerr(self.g_orc32, self.g64))


# ---- the whole sweep: every case, once per section, and the noise of each group ------------------------------------------
SECTIONS = ("forward", "walk", "flow", "backward", "slicing", "train")


class Sweep:
    """Every case of tests/test_gpu_wide_domain.py with its references, built once per section on first use, and `noise`:
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
                if wide_supported(D, L, U) or mfma_supported(D, L, U):
                    self._note(prefix + name, L, c.noise(inverse, "fold32"))
                if generic:
                    self._note("generic " + name, L, c.noise(inverse, "orc32"))

    def _build_forward(self):
        shapes = [s for HT, UT in CELLS for s in forward_cell(HT, UT)] + [NARROW_KEPT]
        self.fwd = {s: WideCase(self.oracle, *s) for s in dict.fromkeys(shapes + [RAW_CELL, MISC_CELL])}
        self._directions(list(self.fwd.items()))

    def _build_walk(self):
        M, _, N = WALK_ROWS[0]
        self.walk = {HT: WideCase(self.oracle, *walk_shape(HT), rows=(M, N), blocks=2, generic=False) for HT in HTS}
        self._directions([(walk_shape(HT), c) for HT, c in self.walk.items()], "tile walk ", generic=False)

    def _build_flow(self):
        self.flow = {s: FlowCase(self.tnf, self.oracle, *s) for s in flow_shapes()}
        for (D, S, L, U), c in self.flow.items():
            for k, v in c.noise().items():
                self._add("flow S%d %s" % (S, k), L, v)

    def _build_backward(self):
        self.bwd = {}
        for D, L, U in backward_shapes():
            for upper, inverse in backward_direction(D, L, U):
                for M, Mp, N in BWD_ROWS:
                    c = self.bwd[(D, L, U, upper, inverse, M, Mp, N)] = GradCase(self.oracle, D, L, U, upper, inverse, M, Mp, N)
                    if backward_route(D, L, U, Mp, N) == "wide":
                        self._note("backward", L, c.noise("fold32"), ("g_z", "g_params"))
                    self._note("generic backward", L, c.noise("orc32"), ("g_z", "g_params"))

    def _build_slicing(self):
        D, L, U = SLICE_CELL
        self.slices = {N: GradCase(self.oracle, D, L, U, True, True, 1, 1, N, generic=False) for N in SLICE_NS}
        for c in self.slices.values():
            self._note("sliced backward", L, c.noise("fold32"), ("g_z", "g_params"))

    def _build_train(self):
        self.train = {s: TrainCase(self.tnf, self.oracle, *s) for s in TRAIN_SHAPES}
        for (D, S, L, U), c in self.train.items():
            self._add("unfused flow backward g_params", L, c.noise())

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
        for key, sec in (("tile walk", "walk"), ("unfused", "train"), ("flow ", "flow"), ("sliced", "slicing"),
                         ("backward", "backward")):
            if key in name:
                return sec
        return "forward"
