"""numpy restatement of the Hebbian learning-rule simulator (include/tnf_hebb.h), written from the header's text and
vectorised over the simulations.  Everything takes `dtype`: np.float64 is the reference; np.float32 is the TWIN -- every
product, sum and difference rounded one by one, as the kernel rounds them -- whose distance from float64 sets the tests'
bars.  The one freedom of the contract, the association of the dot product y, is a parameter: `order` = "forward",
"reverse" or "stride4" (four interleaved partial sums, k mod 4, added pairwise at the end).  Nothing here imports the
package.  tests/golden/hebb.npz (tools/gen_hebb_golden.py) pins `simulate` to the reference notebook's own function."""
import numpy as np

ORDERS = ("forward", "reverse", "stride4")


def dot_rows(w, xr, order="forward"):
    """y_i = sum_k w[i, k] * xr[k] in w's dtype, products rounded, added in the named order."""
    p = w * xr[None, :]
    n = p.shape[1]
    if order == "forward":
        ks = range(n)
    elif order == "reverse":
        ks = range(n - 1, -1, -1)
    elif order == "stride4":
        parts = []
        for c in range(min(4, n)):
            acc = p[:, c].copy()
            for k in range(c + 4, n, 4):
                acc = acc + p[:, k]
            parts.append(acc)
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        return parts[0]
    else:
        raise ValueError("order must be one of %s" % (ORDERS,))
    ks = list(ks)
    acc = p[:, ks[0]].copy()
    for k in ks[1:]:
        acc = acc + p[:, k]
    return acc


def step(w, z, xr, omega, sigma_eps, order="forward"):
    """One step from the states w (N, n) with the input row xr (n) and the standard normals omega (N, n); everything
    already in one dtype.  A NaN stays a NaN through the two clips, as in the notebook's masked assignment."""
    f = w.dtype.type
    alpha, beta, theta, b = (z[:, c:c + 1] for c in range(4))
    y = dot_rows(w, xr, order)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        dw = (alpha * y) * (xr[None, :] - theta) - (beta * (y * y)) * w
        w = (w + dw) + f(sigma_eps) * omega
        w = np.where(w < -b, -b, w)
        w = np.where(w > b, b, w)
    return w


def simulate(z, x, w0, eps, sigma_eps, n_steps=None, j0=0, dtype=np.float64, order="forward", keep=None):
    """z (N, 4), x (N_x, n), w0 (n,) / (1, n) / (N, n), eps (n_steps, N, n) standard normals (None: no noise) ->
    (w (N, n), {s: state after step s for s in keep}).  Step s uses row (j0 + s) mod N_x of x."""
    z, x = np.asarray(z).astype(dtype), np.asarray(x).astype(dtype)
    N, N_x = z.shape[0], x.shape[0]
    w = np.broadcast_to(np.asarray(w0).astype(dtype).reshape(-1, x.shape[1]), (N, x.shape[1])).copy()
    if n_steps is None:
        n_steps = eps.shape[0]
    zero = np.zeros((N, x.shape[1]), dtype=dtype)
    kept = {}
    for s in range(n_steps):
        om = zero if eps is None else np.asarray(eps[s]).astype(dtype)
        w = step(w, z, x[(j0 + s) % N_x], om, sigma_eps, order)
        if keep is not None and s in keep:
            kept[s] = w.copy()
    return w, kept


def trajectory(z, x, w0, eps, sigma_eps, n_steps=None, j0=0, dtype=np.float64, order="forward"):
    """The state after every step: (n_steps, N, n)."""
    n_steps = eps.shape[0] if n_steps is None else n_steps
    _, kept = simulate(z, x, w0, eps, sigma_eps, n_steps, j0, dtype, order, keep=set(range(n_steps)))
    return np.stack([kept[s] for s in range(n_steps)])


def row_err(got, want, b):
    """max_k |got - want| / b per row: the error measure of the Hebbian tests.  got, want (..., N, n), b (N,) -> (..., N);
    a row where one side is non-finite and the other is not counts as inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
    d = np.where(np.isnan(got) & np.isnan(want), 0.0, np.where(np.isfinite(d), d, np.inf))
    return d.max(axis=-1) / np.asarray(b, dtype=np.float64)


def prior_rows(rng, N, box=None):
    """N parameter rows from a RandomState: the whole prior of the notebook's SNPE_prior round 1 (box None), or a benign
    group -- "box": alpha, beta log-uniform on [1e-5, 1e-2], theta_x in (-3, 3), b in (1, 20); "clip": the same with
    b in (0.2, 1.5)."""
    hi = -1.0 if box is None else -2.0
    b_lo, b_hi = (0.2, 1.5) if box == "clip" else (1.0, 20.0)
    return np.stack((10.0 ** rng.uniform(-5, hi, N), 10.0 ** rng.uniform(-5, hi, N), rng.uniform(-3, 3, N),
                     rng.uniform(b_lo, b_hi, N)), axis=1)


def inputs(rng, n, N_x):
    """(x (N_x, n), w0 (n,)) as systems.HebbLearn draws them, from a RandomState."""
    df = 5 * n
    A = rng.normal(0, 1, (df, n))
    Sigma = np.linalg.inv(A.T @ A / df)  # IW(df, df I): the inverse of a Wishart(df, I / df)
    return rng.multivariate_normal(np.zeros(n), Sigma, N_x), rng.normal(0, 1, n)
