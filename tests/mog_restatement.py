"""A dtype-generic torch restatement of the reference's MoG arithmetic (density_estimator.py:90-213), op for op: it
builds U, forms Sigma_inv = U^T U, takes the quadratic form as two matmuls and has both branches (K == 1, K > 1) with
their EPS terms.  tests/test_mog_host.py pins it to the reference's recorded outputs (tests/golden/mog.npz); the GPU
tests then use it, in float64, as their oracle and, in float32 on the CPU, as the measure of the reference's own noise.
A helper like tests/split_f16_emulation.py: no test in here.

Like the reference, the bound constants m = (ub - lb)/2 and c = (ub + lb)/2 are float32 tensors whatever the dtype of
params: sqrt(m) is taken in float32, the products promote."""
import numpy as np
import torch

EPS = 1e-12


def mog_params(params, D, K, lb=None, ub=None):
    """(alpha (M, K), mu (M, K, D), Sigma_inv (M, K, D, D), Sigma_det (M, K)) in params' dtype."""
    M, T = params.shape[0], D * (D + 1) // 2
    bounded = lb is not None and ub is not None
    alpha = torch.softmax(params[:, :K], dim=1)
    mu = params[:, K:K + K * D].view(-1, K, D)
    if bounded:
        m = torch.tensor((np.asarray(ub) - np.asarray(lb)) / 2.0).float()[None, None, :]
        c = torch.tensor((np.asarray(ub) + np.asarray(lb)) / 2.0).float()[None, None, :]
        mu = m * torch.tanh(mu) + c
    packed = params[:, K + K * D:K + K * D + K * T].view(-1, K, T)
    U = torch.zeros((M, K, D, D), dtype=params.dtype)
    inds = torch.triu_indices(D, D)
    U[:, :, inds[0], inds[1]] = packed
    diag_in = U[:, :, range(D), range(D)]
    diag = torch.exp(diag_in)
    if bounded:
        diag = diag / torch.sqrt(m)
    U[:, :, range(D), range(D)] = diag
    Sigma_inv = torch.matmul(torch.transpose(U, 3, 2), U)
    if bounded:
        Sigma_det = torch.prod(m * torch.exp(-2.0 * diag_in), dim=2)
    else:
        Sigma_det = torch.prod(torch.exp(-2.0 * diag_in), dim=2)
    return alpha, mu, Sigma_inv, Sigma_det


def log_prob(z, params, D, K, lb=None, ub=None):
    """z (M_z, N, D), params (M_p, D_params), broadcasting as torch does -> (M, N)."""
    alpha, mu, Sigma_inv, Sigma_det = mog_params(params, D, K, lb, ub)
    if K == 1:
        d = z - mu
        q = torch.matmul(torch.matmul(d[:, :, None, :], Sigma_inv), d[:, :, :, None])[:, :, 0, 0]
        q = q + torch.log(Sigma_det + EPS)
        q = q + D * np.log(2.0 * np.pi)
        return -0.5 * q
    d = z[:, :, None, :] - mu[:, None, :, :]
    q = torch.matmul(torch.matmul(d[:, :, :, None, :], Sigma_inv[:, None, :, :, :]), d[:, :, :, :, None])
    num = torch.exp(-0.5 * q)
    den = torch.sqrt(((2 * np.pi) ** D) * Sigma_det + EPS)[:, None, :]
    prob = torch.sum(alpha[:, None, :] * (num[:, :, :, 0, 0] / den), dim=2)
    return torch.log(prob + EPS)


def sample_map(params, u, e1, e2, D, K, lb=None, ub=None):
    """The sampling map of MoG._forward_from in params' dtype: k = #{j : cumsum(alpha)_j <= u} (at most K - 1),
    z = mu_k + U_k^-1 e1 + sqrt(0.001) e2.  Returns (z, k, distance of u to the nearest cumulative-alpha boundary)."""
    alpha, mu, Sigma_inv, _ = mog_params(params, D, K, lb, ub)
    cum = torch.cumsum(alpha, dim=1)[:, None, :]                               # (M, 1, K)
    k = (cum <= u[:, :, None]).sum(2).clamp(max=K - 1)                          # (M, N)
    gap = (cum[:, :, :K - 1] - u[:, :, None]).abs().amin(2) if K > 1 else torch.ones_like(u)
    U = torch.linalg.cholesky(Sigma_inv, upper=True)                            # the factor with its positive diagonal
    idx = k[:, :, None, None].expand(-1, -1, D, D)
    Uk = torch.gather(U[:, None].expand(-1, u.shape[1], -1, -1, -1), 2, idx[:, :, None]).squeeze(2)
    muk = torch.gather(mu[:, None].expand(-1, u.shape[1], -1, -1), 2, k[:, :, None, None].expand(-1, -1, 1, D)).squeeze(2)
    x = torch.linalg.solve_triangular(Uk, e1[..., None], upper=True)[..., 0]
    return muk + x + (0.001 ** 0.5) * e2, k, gap
