"""What the whole-flow wide tests share (tests/test_wideflow_host.py, tests/test_gpu_wideflow.py): the formulation of
csrc/flow_wide.hip + wide_flow_tile.h restated in torch (in the dtype of its inputs), its LDS formula and support predicate
restated, the sweep's grid, its fixed inputs and its float64 references.  A helper like tests/wide_restatement.py: no
test in here.

The kernel carries a row as two register halves of 16 HT slots -- lo = features 0 .. h-1, hi = features h .. D-1,
h = D // 2, zero above the real width -- and walks the 2 S coupling layers on them in the folded formulation of
wide_restatement.folded_coupling, generalised to a layer d_in -> U -> ... -> U -> d_out whose widths differ (odd D) and are
zero-padded to 16 HT and 16 UT.  Between layers both halves take v -> v A + B with (A, B) = (1, 0) at a padded slot.  The
padded slots are part of what is restated: log_prob sums z0^2 over all 32 HT slots, as the kernel does."""
import torch

from domain_helpers import float64
from maf_restatement import HALF_LOG_2PI, LN2, LOG2E, err, weight_scale  # noqa: F401 -- err: used by the tests
from wide_restatement import _bmm, _sig2, stats_list

LDS_BUDGET = 150 * 1024  # kWideFlowLdsBudget
WAVES, GRID_BUDGET = 8, 256  # WF_WAVES; persistent_bx(tiles, WF_WAVES, 256, M)


# ---- the predicate -------------------------------------------------------------------------------------------------------
def tiles(D, U):
    return ((D + 1) // 2 + 15) // 16, (U + 15) // 16


def layer_floats(D, L, U):
    """One coupling layer's share of the LDS: WideLayout{UT, HT, L}.floats() + the fold block of 64 HT floats."""
    HT, UT = tiles(D, U)
    return (4 * HT * UT + (L - 1) * 2 * UT * UT) * 256 + (2 * L * UT + 2 * HT) * 16 + 64 * HT


def lds_bytes(D, S, L, U):
    return 4 * 2 * S * layer_floats(D, L, U)


def wide_flow_supported(D, S, L, U):
    return 2 <= D <= 64 and S >= 1 and 1 <= L <= 5 and 17 <= U <= 64 and lds_bytes(D, S, L, U) <= LDS_BUDGET


def largest_S(D, L, U):
    return LDS_BUDGET // lds_bytes(D, 1, L, U)


def grid_x(N, M):
    return min(((N + 15) // 16 + WAVES - 1) // WAVES, max(1, GRID_BUDGET // M))


# ---- the layout of a parameter row (any D) -----------------------------------------------------------------------------------
def coupling_dims(D, upper):
    h = D // 2
    return (h, D - h) if upper else (D - h, h)


def coupling_params(D, L, U, upper):
    d_in, d_out = coupling_dims(D, upper)
    return 2 * (d_in * U + d_out * U + d_out + U + (L - 1) * (U + 1) * U)


def flow_params(D, S, L, U):
    return S * (coupling_params(D, L, U, True) + coupling_params(D, L, U, False) + 2 * D)


def _stage(D, L, U):
    up, low = coupling_params(D, L, U, True), coupling_params(D, L, U, False)
    return up, low, up + low + 2 * D


def layer_row(params, D, L, U, c):
    up, low, stage = _stage(D, L, U)
    off = (c >> 1) * stage + (c & 1) * up
    return params[:, off:off + (low if c & 1 else up)]


def affine_row(params, D, L, U, st):
    up, low, stage = _stage(D, L, U)
    off = st * stage + up + low
    return params[:, off:off + D], params[:, off + D:off + 2 * D]


# ---- the folded formulation on padded halves ------------------------------------------------------------------------------------
def _pad_to(x, n):
    return torch.nn.functional.pad(x, (0, n - x.shape[-1]))


def _image(row, d_in, d_out, L, U, HT, UT, pad_weight):
    """[(W_t, W_s, b_t, b_s)] of a layer's packed row, every matrix zero-padded to the tile multiples of the operand image.
    `pad_weight` (a planted defect): the t-net's output bias of the first padded slot is 0.25 instead of 0."""
    dims, pads = [d_in] + [U] * L + [d_out], [16 * HT] + [16 * UT] * L + [16 * HT]
    out, off = [], 0
    for i in range(L + 1):
        di, do = dims[i], dims[i + 1]
        w, b = [], []
        for _ in range(2):
            w.append(row[:, off:off + di * do].reshape(-1, di, do))
            off += di * do
        for _ in range(2):
            b.append(row[:, off:off + do].reshape(-1, 1, do))
            off += do
        w = [torch.nn.functional.pad(x, (0, pads[i + 1] - do, 0, pads[i] - di)) for x in w]
        b = [_pad_to(x, pads[i + 1]) for x in b]
        if pad_weight and i == L and do < pads[i + 1]:
            b[0] = b[0].clone()
            b[0][..., do] = 0.25
        out.append((w[0], w[1], b[0], b[1]))
    assert off == row.shape[1]
    return out


def folded_layer(x, y, W, L, inverse):
    """wide_flow_layer: conditioner half x, transformed half y (16 HT slots each) -> (y', sum of s' over the slots)."""
    c = 2.0 * LOG2E
    wt, ws, bt, bs = W[0]
    r = [_sig2(c * bt + _bmm(x, c * wt)), _sig2(c * bs + _bmm(x, c * ws))]
    for l in range(1, L):
        r = [_sig2(c * (b + w.sum(1, keepdim=True)) + _bmm(r[n], (-2.0 * c) * w)) for n, (w, b) in enumerate(zip(W[l][:2], W[l][2:]))]
    wt, ws, bt, bs = W[L]
    t = (bt + wt.sum(1, keepdim=True)) + _bmm(r[0], -2.0 * wt)
    s2 = LOG2E * (bs + ws.sum(1, keepdim=True)) + _bmm(r[1], (-2.0 * LOG2E) * ws)
    y = y.expand(t.shape[0], -1, -1)
    return ((y - t) * torch.exp2(-s2) if inverse else y * torch.exp2(s2) + t), s2.sum(2)


def fold_block(params, D, L, U, stat, c, inverse, HT, pad_fold=False):
    """The fold block of layer c -> (A_lo, A_hi, B_lo, B_hi), each (M_p, 1, 16 HT), and the layer's constant log-det (M_p, 1):
    fold_consts of coupling_mfma.hip on the real slots, (1, 0) on the padded ones.  `pad_fold` (a planted defect): B = 0.25
    at the padded slots."""
    mean, alpha = (s[c].to(params.dtype).reshape(1, 1, D) for s in stat)
    ld = -torch.log(alpha).sum().reshape(1, 1).expand(params.shape[0], 1)
    ea, shift = torch.ones_like(alpha), torch.zeros_like(alpha)
    if c & 1:
        a, shift = (v[:, None] for v in affine_row(params, D, L, U, c >> 1))
        ld, ea = ld + a.sum(2), torch.exp(a)
    if inverse:
        A = alpha / ea
        B = mean - shift * A
    else:
        A = ea / alpha
        B = shift - mean * A
    A, B = A.expand(params.shape[0], 1, D), B.expand(params.shape[0], 1, D)
    h, n = D // 2, 16 * HT

    def padded(v, fill):
        return torch.cat((v, torch.full(v.shape[:2] + (n - v.shape[2],), fill, dtype=v.dtype)), 2)

    fill_b = 0.25 if pad_fold else 0.0
    return padded(A[..., :h], 1.0), padded(A[..., h:], 1.0), padded(B[..., :h], fill_b), padded(B[..., h:], fill_b), ld


def _halves(z, D, HT):
    h = D // 2
    return _pad_to(z[..., :h], 16 * HT), _pad_to(z[..., h:], 16 * HT)


def _join(lo, hi, D):
    h = D // 2
    return torch.cat((lo[..., :h], hi[..., :D - h]), 2)


def _walk(z, params, D, S, L, U, stat, inverse, defect):
    HT, UT = tiles(D, U)
    lo, hi = _halves(z, D, HT)
    M = max(z.shape[0], params.shape[0])
    lo, hi = lo.expand(M, -1, -1), hi.expand(M, -1, -1)
    ssum, ldc = 0.0, 0.0
    for c in (reversed(range(2 * S)) if inverse else range(2 * S)):
        upper = c % 2 == 0
        W = _image(layer_row(params, D, L, U, c), *coupling_dims(D, upper), L, U, HT, UT, defect == "pad_weight")
        Al, Ah, Bl, Bh, ld = fold_block(params, D, L, U, stat, c, inverse, HT, defect == "pad_fold")
        ldc = ldc + ld
        if inverse:
            lo, hi = lo * Al + Bl, hi * Ah + Bh
        if upper:
            hi, s = folded_layer(lo, hi, W, L, inverse)
        else:
            lo, s = folded_layer(hi, lo, W, L, inverse)
        ssum = ssum + s
        if not inverse:
            lo, hi = lo * Al + Bl, hi * Ah + Bh
    return lo, hi, LN2 * ssum + ldc


def wide_flow_log_prob(z, params, D, S, L, U, stat, defect=None):
    """tnf_wide_flow_log_prob_f32 restated -> (log_prob, z0, sum_log_det).  stat = (mean (2S, D), alpha (2S, D));
    z (M_z, N, D), params (M_p, P), M's in {1, M}.  defect: None, "pad_weight" or "pad_fold"."""
    lo, hi, sld = _walk(z, params, D, S, L, U, stat, True, defect)
    sq = (lo * lo).sum(2) + (hi * hi).sum(2)  # over every slot: the padding is part of the claim
    return -0.5 * sq - D * HALF_LOG_2PI - sld, _join(lo, hi, D), sld


def wide_flow_forward(omega, params, D, S, L, U, stat, defect=None):
    """tnf_wide_flow_forward_f32 restated -> (z, sum_log_det, the largest |padded slot|)."""
    lo, hi, sld = _walk(omega, params, D, S, L, U, stat, False, defect)
    h = D // 2
    pad = max(float(lo[..., h:].abs().max()) if lo.shape[2] > h else 0.0,
              float(hi[..., D - h:].abs().max()) if hi.shape[2] > D - h else 0.0)
    return _join(lo, hi, D), sld, pad


# ---- the grid ------------------------------------------------------------------------------------------------------------
DS = {1: (2, 3, 5, 8, 31, 32), 2: (33, 63, 64)}
US = {2: (17, 20, 32), 3: (33, 48), 4: (64,)}
ROWS = [(1, 1, 1), (1, 1, 15), (1, 1, 16), (1, 1, 17), (1, 1, 33), (3, 3, 33), (3, 1, 33)]
LP_ONLY_ROWS = [(1, 3, 33)]
M_FULL, N_FULL = 3, 33
WALK_N, WALK_M = 2065, 512  # 130 tiles, the last with one row
WALK_SHAPES = {1: (5, 1, 2, 20), 2: (33, 1, 2, 20)}
L5_SHAPE = (8, 1, 5, 20)
CDE_SHAPE = (4, 1, 2, 20)  # NormFlow(4, True, 'coupling', 1, 2, 20): the reference's own conditional-flow test


def sweep_shapes(refused=False):
    """(D, S, L, U): one case per (HT, UT, L in 1 .. 3) cell, D, U and S cycling through their lists (S through 1, 2 and
    the largest supported, never above it), and L = 5 at one cell.  A cell whose two images do not fit the LDS even at
    S = 1 (UT = 4 with L = 3) has no case: `refused` lists those cells' shapes at S = 1 instead."""
    out, no, i = [], [], 0
    for HT in (1, 2):
        for UT in (2, 3, 4):
            for L in (1, 2, 3):
                D, U = DS[HT][i % len(DS[HT])], US[UT][(i // 3 + L) % len(US[UT])]
                assert tiles(D, U) == (HT, UT)
                top = largest_S(D, L, U)
                i += 1
                if top < 1:
                    no.append((D, 1, L, U))
                    continue
                S = min((1, 2, top)[(i + HT) % 3], top)
                assert wide_flow_supported(D, S, L, U)
                out.append((D, S, L, U))
    return no if refused else out + [L5_SHAPE]


def case_id(shape):
    return "D%d-S%d-L%d-U%d" % shape


# ---- the fixed inputs and their references ----------------------------------------------------------------------------------
SEEDS = 12
LAYOUTS = [(1, 1), (3, 3), (3, 1), (1, 3)]  # (M_z, M_p): every row of ROWS is a slice in N of one of them


class Case:
    """One flow problem under the sweep's law: RealNVP weights and biases ~ N(0, weight_scale(U)) (divided by sqrt(S) from
    S = 3), Affine a ~ N(0, 0.05), shift ~ N(0, 0.1), statistics as domain_helpers._cde draws them (mean ~ 0.1 N(0, 1),
    alpha ~ U(0.75, 1.25)), z = omega ~ N(0, 1): the first of SEEDS seeds whose float64 z0 and frozen z stay below 1e3 in
    every layout.  No seed qualifying is an error."""

    def __init__(self, oracle, D, S, L, U, rows=(M_FULL, N_FULL), layouts=LAYOUTS):
        self.shape, self.oracle, self.rows, self.layouts = (D, S, L, U), oracle, rows, layouts
        assert flow_params(D, S, L, U) == oracle.flow_num_params(D, S, L, U)
        for self.seed in range(SEEDS):
            self._draw(9000 * D + 90 * U + 10 * L + S + 100000 * self.seed)
            try:
                self._ref = {lay: self._f64(*lay) for lay in layouts}
                break
            except OverflowError:
                continue
        else:
            raise RuntimeError("no seed of %d keeps %s below 1e3" % (SEEDS, case_id(self.shape)))
        self._fold = {}

    def _draw(self, seed):
        D, S, L, U = self.shape
        g = torch.Generator().manual_seed(seed)
        R, soften = self.rows[0], S ** -0.5 if S >= 3 else 1.0
        n_w = coupling_params(D, L, U, True) + coupling_params(D, L, U, False)
        stage = [torch.cat((torch.randn(R, n_w, generator=g) * (weight_scale(U) * soften),
                            torch.randn(R, D, generator=g) * 0.05, torch.randn(R, D, generator=g) * 0.1), 1) for _ in range(S)]
        self.params = torch.cat(stage, 1)
        self.stat = (torch.randn(2 * S, D, generator=g) * 0.1, torch.rand(2 * S, D, generator=g) * 0.5 + 0.75)
        self.z = torch.randn(R, self.rows[1], D, generator=g)

    def inputs(self, Mz, Mp, N=None):
        return self.z[:Mz, :N], self.params[:Mp]

    def _f64(self, Mz, Mp):
        z, p = self.inputs(Mz, Mp)
        M = max(Mz, Mp)
        z, p = z.expand(M, -1, -1), p.expand(M, -1)  # the oracle does not broadcast the M's
        with float64(), torch.no_grad():
            st = stats_list(self.stat, torch.float64)
            z0, sld = self.oracle.flow_inverse(z.double(), p.double(), *self.shape, st)
            lp = self.oracle.flow_log_prob(z.double(), p.double(), *self.shape, st)
            out = dict(lp=lp, z0=z0, sld=sld.double())
            if Mz >= Mp:  # sampling: one block of draws per row, or one shared row
                zf, lq, _ = self.oracle.flow_forward(z.double().numpy(), p.double(), *self.shape, st)
                out.update(zf=zf, sldf=torch.tensor(self.oracle.base_log_density_f64(z.double().numpy())) - lq)
        assert all(t.dtype == torch.float64 for t in out.values())
        if not all(bool(torch.isfinite(t).all()) for t in out.values()) or max(
                float(out[k].abs().max()) for k in ("z0", "zf") if k in out) >= 1e3:
            raise OverflowError
        return out

    def want(self, Mz, Mp, N):
        """{quantity: float64 reference} of the row layout (M_z, M_p, N)."""
        return {k: v[:, :N] for k, v in self._ref[(Mz, Mp)].items()}

    def scale(self):
        """{quantity: max(1, max |want|) over the layouts}: the case's denominators of `err`."""
        return {k: max(1.0, *(float(r[k].abs().max()) for r in self._ref.values() if k in r)) for k in ("lp", "z0", "sld", "zf", "sldf")}

    def fold32(self, Mz, Mp):
        """The float32 restatement on the layout's inputs."""
        if (Mz, Mp) not in self._fold:
            z, p = self.inputs(Mz, Mp)
            with torch.no_grad():
                lp, z0, sld = wide_flow_log_prob(z, p, *self.shape, self.stat)
                out = dict(lp=lp, z0=z0, sld=sld)
                if Mz >= Mp:
                    zf, sldf, _ = wide_flow_forward(z, p, *self.shape, self.stat)
                    out.update(zf=zf, sldf=sldf)
            self._fold[(Mz, Mp)] = out
        return self._fold[(Mz, Mp)]

    def noise(self):
        """{quantity: the float32 restatement's error against the float64 oracle, the largest over the layouts}."""
        sc = self.scale()
        out = {}
        for lay in self.layouts:
            for k, got in self.fold32(*lay).items():
                out[k] = max(out.get(k, 0.0), err(got, self._ref[lay][k], sc[k]))
        return out
