"""numpy emulation of the two changes to the whole-flow layer body (f16_tile2.h: TNF2_PSPLIT, TNF2_LDMFMA), beside
tests/split_f16_emulation.py.  No GPU.  Also runs as a script: python tests/test_split_f16_body_emulation.py

1. The split at the production site.  A layer's output y' = u * 2^-s is split right where it is produced, the
   remainder y' - (float)hi written over the dead u, instead of in place over y' by the next layer.  Both forms are
   hi = cvt_pk_f16(y'), rem = fma_mix(-(float)hi + y'), lo = cvt_pk_f16(rem) on the same y': emulated instruction by
   instruction (the fma in float64 and rounded once, as the hardware's fused operation does), the packed halves are
   equal bit for bit -- normal values, values beyond the f16 range (hi = +-inf, rem = -+inf) and NaN included.

2. The log-det on the matrix pipe.  sum_f s_f is linear in the s-net's last sigmoid vector r: one more weight row,
   the column sums of the output weights, gives it as a split-f16 contraction accumulated in fp32 through the layers
   (plus the sum of the biases, the accumulator's initial value).  On the golden flows (D = 32, 64) that sum differs
   from the chain of fp32 adds it replaces by no more than the chain differs from the same flow in float64."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_oracle as orc  # noqa: E402
from conftest import load_golden  # noqa: E402

f32, f16 = np.float32, np.float16


# ---- 1. the split -------------------------------------------------------------------------------------------------
def cvt_pk(v):
    """v_cvt_pk_f16_f32: round to nearest even, |v| >= 65520 -> +-inf"""
    with np.errstate(over="ignore"):
        return v.astype(f16)


def fma_mix_remainder(hb, v):
    """v_fma_mix_f32 d, hb(f16), -1.0, v(f32): one fused operation, rounded once"""
    with np.errstate(invalid="ignore"):
        return (hb.astype(np.float64) * -1.0 + v.astype(np.float64)).astype(f32)


def split_in_place(x):
    """the consuming layer's split2r: the remainder overwrites (a copy of) x"""
    reg = x.copy()
    hb = cvt_pk(reg)
    reg[...] = fma_mix_remainder(hb, reg)
    return hb, cvt_pk(reg)


def split_at_production(y, ay, tt, s2):
    """the producing layer: u = fma(y, Ay, -t), y' = u * 2^-s, then the remainder of y' over u; y' itself stays"""
    with np.errstate(over="ignore", invalid="ignore"):
        u = (y.astype(np.float64) * ay.astype(np.float64) - tt.astype(np.float64)).astype(f32)
        yp = (u * np.exp2(-s2).astype(f32)).astype(f32)
    hb = cvt_pk(yp)
    u[...] = fma_mix_remainder(hb, yp)
    return yp, hb, cvt_pk(u)


def bits(h):
    return h.view(np.uint16)


def test_production_site_split_is_bit_identical():
    rng = np.random.RandomState(0)
    n = 1 << 16
    y = rng.normal(0, 1, n).astype(f32) * np.exp2(rng.randint(-30, 18, n)).astype(f32)
    ay = np.exp(rng.normal(0, 0.3, n)).astype(f32)
    tt = rng.normal(0, 1, n).astype(f32)
    s2 = rng.normal(0, 2, n).astype(f32)
    # edge values: the f16 overflow threshold from both sides, subnormal remainders, zeros, infinities, NaN
    edge = np.array([65519.996, 65520.0, -65520.0, 65504.0, 1e5, -3e38, 6e-8, 5.9e-8, 1e-30, 0.0, -0.0, np.inf, -np.inf,
                     np.nan, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12], f32)
    y[:edge.size], ay[:edge.size], tt[:edge.size], s2[:edge.size] = edge, 1.0, 0.0, 0.0
    yp, hi_p, lo_p = split_at_production(y, ay, tt, s2)
    hi_c, lo_c = split_in_place(yp)  # what the next layer did with the same register
    assert np.array_equal(yp[:edge.size], edge, equal_nan=True)  # the edge values reached the split
    assert np.array_equal(bits(hi_p), bits(hi_c)) and np.array_equal(bits(lo_p), bits(lo_c))
    # the remainder is exact wherever hi is finite: x = hi + rem in fp32, so nothing depends on where it is kept
    ok = np.isfinite(hi_p.astype(f32)) & np.isfinite(yp)
    rem = fma_mix_remainder(hi_p, yp)
    assert np.array_equal(hi_p[ok].astype(np.float64) + rem[ok].astype(np.float64), yp[ok].astype(np.float64))
    # out of range: hi = +-inf and the remainder the opposite infinity, which is what makes the products NaN (detected)
    big = np.abs(yp) >= 65520.0
    assert big.any() and np.all(np.isinf(hi_p[big & np.isfinite(yp)].astype(f32)))


# ---- 2. the log-det -----------------------------------------------------------------------------------------------
def split(v):
    v = v.astype(f32)
    hi = v.astype(f16)
    return hi, (v - hi.astype(f32)).astype(f16)


def mm3(x, w):
    """x (N, K), w (K, O) fp32 -> fp32 accumulate of xh wh + xl wh + xh wl (products of f16 values are exact in fp32)"""
    xh, xl = split(x)
    wh, wl = split(w)
    f = lambda a, b: a.astype(f32) @ b.astype(f32)  # noqa: E731
    return f(xh, wh) + f(xl, wh) + f(xh, wl)


def coupling_inverse(z, p, D, L, U, upper, exact):
    """One coupling layer, inverse direction.  exact: float64 throughout (the truth); else the split-f16 emulation.
    Returns z', and the layer's sum of s three ways: (add chain in fp32, column-sum contraction in fp32) or float64."""
    h = D // 2
    z1, z2 = (z[:, :h], z[:, h:]) if upper else (z[:, h:], z[:, :h])
    dt = np.float64 if exact else f32
    mm = (lambda a, b: a @ b) if exact else mm3
    off = 0

    def take(n, shape):
        nonlocal off
        v = p[off:off + n].reshape(shape).astype(dt)
        off += n
        return v

    def layer(xt, xs, din, dout):
        wt, ws = take(din * dout, (din, dout)), take(din * dout, (din, dout))
        bt, bs = take(dout, (dout,)), take(dout, (dout,))
        return mm(xt, wt) + bt, mm(xs, ws) + bs, ws, bs

    t, s, _, _ = layer(z1, z1, h, U)
    t, s = np.tanh(t), np.tanh(s)
    for _ in range(L - 1):
        t, s, _, _ = layer(t, s, U, U)
        t, s = np.tanh(t), np.tanh(s)
    hs = s  # the s-net's last hidden vector
    t, s, ws, bs = layer(t, hs, U, h)
    z2 = (z2 - t) / np.exp(s)
    out = (np.concatenate([z1, z2], 1) if upper else np.concatenate([z2, z1], 1)).astype(dt)
    if exact:
        return out, s.sum(1)
    chain = np.zeros(z.shape[0], f32)
    for f_ in range(h):  # one fp32 add per feature
        chain = chain + s[:, f_]
    colsum = ws.sum(1, dtype=f32).reshape(U, 1)  # built once per layer in the prologue
    row = (mm3(hs, colsum)[:, 0] + bs.sum(dtype=f32)).astype(f32)
    return out, (chain, row)


def flow_sum_s(z, params, D, S, L, U, stats, exact):
    """sum over the coupling layers of sum(s) per sample; BatchNorm / Affine between the layers as in the flow"""
    lay = orc.flow_layout(D, S, L, U)
    idx = sum(n for _, n, _ in lay)
    bi = 2 * S
    dt = np.float64 if exact else f32
    z = z.astype(dt)
    tot = np.zeros(z.shape[0], np.float64) if exact else [np.zeros(z.shape[0], f32), np.zeros(z.shape[0], f32)]
    for kind, n, upper in reversed(lay):
        if kind == "coupling":
            z, ld = coupling_inverse(z, params[idx - n:idx], D, L, U, upper, exact)
            if exact:
                tot = tot + ld
            else:
                tot = [tot[0] + ld[0], tot[1] + ld[1]]  # the kernel carries both forms through the layers in fp32
        elif kind == "affine":
            a, sh = params[idx - n:idx - n + D].astype(dt), params[idx - n + D:idx].astype(dt)
            z = (z - sh) / np.exp(a)
        else:
            bi -= 1
            m, al = stats[bi]
            z = z * al.astype(dt) + m.astype(dt)
        idx -= n
    return tot


def logdet_errors():
    g = load_golden("flow")
    rows = []
    for ci, (D, S, L, U, N) in enumerate(g["meta"].tolist()):
        if D not in (32, 64):
            continue
        k = "f%02d_" % ci
        stats = list(zip(g[k + "bn_mean"], g[k + "bn_alpha"]))
        z, p = g[k + "z_test"][0], g[k + "params"][0]
        truth = flow_sum_s(z, p, D, S, L, U, stats, True)
        chain, row = flow_sum_s(z, p, D, S, L, U, stats, False)
        rows.append((ci, D, S, L, U, float(np.abs(chain - truth).max()), float(np.abs(row - truth).max()),
                     float(np.abs(row.astype(np.float64) - chain).max())))
    return rows


def test_rowsum_logdet_within_the_add_chains_error():
    rows = logdet_errors()
    assert rows, "no D = 32 / 64 flow in tests/golden/flow.npz"
    for ci, D, S, L, U, e_chain, e_row, d in rows:
        print("case %d D=%d S=%d L=%d U=%d: |chain - f64| %.3e  |row - f64| %.3e  |row - chain| %.3e" % (
            ci, D, S, L, U, e_chain, e_row, d))
    worst_chain = max(r[5] for r in rows)
    assert max(r[7] for r in rows) <= worst_chain, "the row sum is further from the add chain than the chain from float64"
    assert max(r[6] for r in rows) <= worst_chain, "the row sum is further from float64 than the add chain"


if __name__ == "__main__":
    test_production_site_split_is_bit_identical()
    print("split at the production site: packed halves bit-identical")
    test_rowsum_logdet_within_the_add_chains_error()
