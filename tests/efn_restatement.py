"""float64 numpy restatement of the EFN prior and KL kernels (include/tnf_efn.h), written from the header's text and
vectorised over the contexts.  Nothing here imports the package.  tests/test_efn_host.py ties `mvn_eta` to the package's
MVN.mu_to_eta (itself pinned to the reference by tests/golden/expfam.npz) and the two KL functions to the reference's own
KL values of that fixture; tests/test_gpu_efn.py compares the kernels with these functions."""
import math

import numpy as np

U24 = 2.0 ** -24  # unit roundoff of float32


def mvn_num_noise(D, df):
    return D * (1 + df)


def mvn_parts(noise, D, df, sigma_mu=1.0):
    """The header's draw order: noise (M, K = D (1 + df)) normals -> mu (M, D), the Bartlett factor L (M, D, D) and
    W = L L^T / df (M, D, D), the precision."""
    noise = np.asarray(noise, dtype=np.float64)
    M = noise.shape[0]
    assert noise.shape == (M, mvn_num_noise(D, df))
    mu = sigma_mu * noise[:, :D]
    L = np.zeros((M, D, D))
    k = D
    for i in range(D):
        L[:, i, :i] = noise[:, k:k + i]
        k += i
    for i in range(D):
        L[:, i, i] = np.sqrt(np.sum(noise[:, k:k + df - i] ** 2, axis=1))
        k += df - i
    assert k == noise.shape[1]
    W = np.matmul(L, np.transpose(L, (0, 2, 1))) / df
    return mu, L, W


def mvn_eta(noise, D, df, sigma_mu=1.0):
    """eta (M, D + D (D + 1) / 2) = [W mu | packed upper triangle, -W_ii / 2 on the diagonal and -W_ij off it]."""
    mu, _, W = mvn_parts(noise, D, df, sigma_mu)
    eta1 = np.matmul(W, mu[:, :, None])[:, :, 0]
    rows, cols = np.triu_indices(D)
    eta2 = np.where(rows == cols, -0.5, -1.0) * W[:, rows, cols]
    return np.concatenate((eta1, eta2), axis=1)


def dirichlet_eta(u, lb, ub):
    """u (M, D) uniforms -> eta = [lb + (ub - lb) u | 1]."""
    u = np.asarray(u, dtype=np.float64)
    return np.concatenate((lb + (ub - lb) * u, np.ones((u.shape[0], 1))), axis=1)


def eta_bar(eta, D, df=None):
    """The kernels' float32 error bar per row: 4 * n_terms * 2^-24 of the row's largest |eta| entry, n_terms the longest
    float32 sum behind an entry -- df terms for a chi-square, D for a row of L L^T or of W mu; one fma for Dirichlet."""
    n_terms = 1 if df is None else max(df, D)
    return 4.0 * n_terms * U24 * np.max(np.abs(eta), axis=1)


def kl_mvn(z, log_q, eta):
    """The kernel's formulation: the precision P from eta2, P = C C^T, mu = P^-1 eta1 by two triangular solves,
    y = C^T (z - mu), log p = -|y|^2 / 2 + sum log C_ii - D/2 log 2 pi.  A precision that is not positive definite
    gives NaN in that row."""
    z, log_q, eta = (np.asarray(a, dtype=np.float64) for a in (z, log_q, eta))
    M, N, D = z.shape
    rows, cols = np.triu_indices(D)
    out = np.full((M,), np.nan)
    for m in range(M):
        P = np.zeros((D, D))
        P[rows, cols] = -eta[m, D:]
        P = P + P.T  # doubles the diagonal: P_ii = -2 eta2_ii, P_ij = -eta2_ij
        try:
            C = np.linalg.cholesky(P)
        except np.linalg.LinAlgError:
            continue
        mu = np.linalg.solve(C.T, np.linalg.solve(C, eta[m, :D]))
        y = np.matmul(z[m] - mu, C)  # rows: (C^T (z - mu))^T
        log_p = -0.5 * np.sum(y * y, axis=1) + np.sum(np.log(np.diag(C))) - 0.5 * D * math.log(2.0 * math.pi)
        out[m] = np.mean(log_q[m] - log_p)
    return out


def kl_dirichlet(z, log_q, eta):
    """z' = (z + 1e-32) / sum(z + 1e-32), log p = lgamma(sum alpha) - sum lgamma(alpha_i) + sum (alpha_i - 1) log z'_i."""
    z, log_q, eta = (np.asarray(a, dtype=np.float64) for a in (z, log_q, eta))
    M, N, D = z.shape
    zp = z + 1e-32
    zp = zp / np.sum(zp, axis=2, keepdims=True)
    out = np.zeros((M,))
    for m in range(M):
        alpha = eta[m, :D]
        const = math.lgamma(float(np.sum(alpha))) - sum(math.lgamma(float(a)) for a in alpha)
        out[m] = np.mean(log_q[m] - (const + np.sum((alpha - 1.0) * np.log(zp[m]), axis=1)))
    return out
