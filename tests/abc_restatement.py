"""numpy restatement of the rejection-ABC kernels (include/tnf_abc.h), written from the header's text: the counter-based
stream (Philox4x32-10 in uint64 arithmetic, Box-Muller), the truncated-Gaussian proposal, Mat's statistics and the chain.
Everything takes `dtype`: np.float64 is the reference; np.float32 is the TWIN -- the same arithmetic in the kernel's
order and number format (products and sums rounded one by one, LU with the kernel's compare-and-select pivoting) -- whose
distance from float64 sets the tests' bars.  Nothing here imports the package."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC 2011): counters and key as broadcastable integer arrays ->
    four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & MASK for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _pair(wa, wb, dtype):
    f = dtype
    # float32: the sum rounds to even from 2^23 on, as the kernel's float add does; exact in float64
    u1 = ((wa >> np.uint32(8)).astype(f) + f(0.5)) * f(2.0 ** -24)
    u2 = (wb >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    r = np.sqrt(f(-2.0) * np.log(u1))
    ang = f(2.0 * np.pi) * u2
    return r * np.cos(ang), r * np.sin(ang)


def normals(seed, t, i, j, D, dtype=np.float64):
    """omega[..., k] = normal k of trial j of chain i in round t: i, j broadcastable integer arrays -> (..., D)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    i, j = np.broadcast_arrays(np.asarray(i), np.asarray(j))
    out = np.empty(i.shape + (4 * ((D + 3) // 4),), dtype=dtype)
    for b in range((D + 3) // 4):
        w = philox4x32(j, t, i, b, k0, k1)
        out[..., 4 * b], out[..., 4 * b + 1] = _pair(w[0], w[1], dtype)
        out[..., 4 * b + 2], out[..., 4 * b + 3] = _pair(w[2], w[3], dtype)
    return out[..., :D]


def noise_block(seed, t, i0, n_i, j0, n_j, D, dtype=np.float64):
    """What tnf_abc_noise_f32 writes: (n_i, n_j, D)."""
    return normals(seed, t, np.arange(i0, i0 + n_i)[:, None], np.arange(j0, j0 + n_j)[None, :], D, dtype)


def candidates(mu, L, omega, dtype=np.float64):
    """z = mu + L omega in the kernel's order (z_r = mu_r + sum_{k <= r} L_rk omega_k, k ascending):
    mu (N, D) or (1, D), L (D, D), omega (N, J, D) -> (N, J, D)."""
    mu, L, omega = (np.asarray(v).astype(dtype) for v in (mu, L, omega))
    D = L.shape[0]
    z = np.empty(omega.shape, dtype=dtype)
    for r in range(D):
        acc = np.broadcast_to(mu[:, None, r], omega.shape[:2]).copy()
        for k in range(r + 1):
            acc = acc + L[r, k] * omega[..., k]
        z[..., r] = acc
    return z


def in_box(z, lb, ub):
    return np.all((np.asarray(lb).astype(z.dtype) < z) & (z < np.asarray(ub).astype(z.dtype)), axis=-1)


def _tri(i, j, d):
    return i * d - i * (i - 1) // 2 + (j - i)


def matrices(z, d):
    z = np.asarray(z)
    A = np.empty(z.shape[:-1] + (d, d), dtype=z.dtype)
    for i in range(d):
        for j in range(i, d):
            A[..., i, j] = A[..., j, i] = z[..., _tri(i, j, d)]
    return A


def stats(z, d, dtype=np.float64):
    """(det A(z), trace A(z)): float64 by LAPACK; the float32 twin by the kernel's LU (the column's largest entry is
    brought up by compare-and-select swaps with each row below in turn, the pivot's reciprocal multiplies)."""
    A = matrices(np.asarray(z).astype(dtype), d)
    tr = A[..., 0, 0].copy()
    for i in range(1, d):
        tr = tr + A[..., i, i]
    if dtype == np.float64:
        return np.stack((np.linalg.det(A), tr), axis=-1)
    a = [[A[..., r, c].copy() for c in range(d)] for r in range(d)]
    det = np.ones(tr.shape, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(d):
            for r in range(c + 1, d):
                sw = np.abs(a[r][c]) > np.abs(a[c][c])
                for k in range(c, d):
                    x, y = a[c][k], a[r][k]
                    a[c][k], a[r][k] = np.where(sw, y, x), np.where(sw, x, y)
                det = np.where(sw, -det, det)
            p = a[c][c]
            det = det * p
            inv = np.where(p != 0, dtype(1.0) / p, dtype(0.0)).astype(dtype)
            for r in range(c + 1, d):
                f = a[r][c] * inv
                for k in range(c + 1, d):
                    a[r][k] = a[r][k] - f * a[c][k]
    return np.stack((det, tr), axis=-1)


def first_accepted(ok):
    """ok (N, J) -> 1-based index of the first True of each row, 0 for a row without one."""
    return np.where(ok.any(axis=1), ok.argmax(axis=1) + 1, 0).astype(np.int32)


def smc_round(mu, L, lb, ub, x0, eps_t, omega, d, dtype=np.float64):
    """One round of every chain from the means mu (N, D) with the noise omega (N, J, D): a dict of the candidates z
    (N, J, D), their statistics x (N, J, 2), the box test, the acceptance test ok (N, J) and trials (N)."""
    z = candidates(mu, L, omega, dtype)
    box = in_box(z, lb, ub)
    x = stats(z, d, dtype)
    with np.errstate(invalid="ignore"):
        near = np.all(np.abs(x - np.asarray(x0).astype(dtype)) < np.asarray(eps_t).astype(dtype), axis=-1)
    ok = box & near
    return dict(z=z, x=x, box=box, ok=ok, trials=first_accepted(ok))


def smc_chain(z0, L, lb, ub, x0, eps, d, max_trials, omega=None, seed=None, dtype=np.float64):
    """All T rounds: -> zs (T, N, D), xs (T, N, 2), trials (T, N); omega (T, N, max_trials, D) or the restated stream.
    An exhausted chain has NaN rows and trials 0 from that round on."""
    z0, eps = np.asarray(z0).astype(dtype), np.asarray(eps)
    N, D = z0.shape
    T = eps.shape[0]
    zs, xs = np.full((T, N, D), np.nan, dtype=dtype), np.full((T, N, 2), np.nan, dtype=dtype)
    trials = np.zeros((T, N), dtype=np.int32)
    mu, alive = z0.copy(), np.ones(N, dtype=bool)
    for t in range(T):
        om = omega[t] if omega is not None else noise_block(seed, t, 0, N, 0, max_trials, D, dtype)
        with np.errstate(invalid="ignore"):
            r = smc_round(np.where(alive[:, None], mu, 0), L, lb, ub, x0, eps[t], om, d, dtype)
        won = alive & (r["trials"] > 0)
        idx = np.maximum(r["trials"] - 1, 0)
        rows = np.arange(N)
        zs[t, won], xs[t, won] = r["z"][rows, idx][won], r["x"][rows, idx][won]
        trials[t, won] = r["trials"][won]
        mu = np.where(won[:, None], r["z"][rows, idx], mu)
        alive = won
    return zs, xs, trials


def propose(mu, L, lb, ub, omega, dtype=np.float64):
    """The truncated draw alone: mu (1, D) or (M, D), omega (M, J, D) -> z (M, D) (NaN rows where no trial is inside),
    trials (M), and the candidates and box test."""
    z = candidates(mu, L, omega, dtype)
    box = in_box(z, lb, ub)
    trials = first_accepted(box)
    out = np.where((trials > 0)[:, None], z[np.arange(z.shape[0]), np.maximum(trials - 1, 0)], np.nan)
    return out, trials, z, box


def rel_err(got, want, scale=None):
    """max |got - want| / max(1, max |want|): the repository's error measure (`scale`: the values the denominator's
    maximum is taken over, when that is a larger set than `want`)."""
    want = np.asarray(want, dtype=np.float64)
    ref = want if scale is None else np.asarray(scale, dtype=np.float64)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)) / max(1.0, float(np.max(np.abs(ref)))))
