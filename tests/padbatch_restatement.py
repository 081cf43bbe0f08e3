"""Sampling with fresh batch statistics through the embedded flow (include/tnf_padbatch.h), restated on the float64
oracle: the oracle's coupling and Affine layers at width 2H on embedded inputs, the oracle's BatchNorm on the REAL
columns only -- a padded column keeps (mean, alpha) = (0, 1), adds nothing to the log-det and is never divided by
sqrt(0 + eps).  TEST INFRASTRUCTURE ONLY; the layout helpers are the restated ones of test_padded_train_host.py."""
import numpy as np
import torch

from test_padded_train_host import embed_features, embed_row, half


def oracle_eps(eps):
    """torch's batch_norm refuses eps = 0 (tests/bn_restatement.py).  1e-30 is below the double rounding of every variance
    met here (> 1e-6): var + 1e-30 == var, so with it the oracle evaluates the expression eps = 0 stands for -- on a real
    column.  On a zero column it would give alpha = 1e-15: the restatement must never get there."""
    return eps if eps > 0 else 1e-30


def flow_forward_eps(omega, params, D, S, L, U, eps, oracle):
    """oracle.flow_forward with batch statistics and BatchNorm's eps as an argument (the oracle fixes 1e-5): the same
    pieces in the same order -> (z, log_q float64, [(mean, alpha)])."""
    z = torch.tensor(omega).to(torch.get_default_dtype())
    log_q = torch.tensor(oracle.base_log_density_f64(omega))
    idx, stats = 0, []
    for kind, n, upper in oracle.flow_layout(D, S, L, U):
        if kind == "coupling":
            z, ld = oracle.coupling(z, params[:, idx:idx + n], D, L, U, upper, False)
        elif kind == "affine":
            z, ld = oracle.affine(z, params[:, idx:idx + n], D, False)
        else:
            z, ld, mean, alpha = oracle.bn_forward_batch(z, eps=oracle_eps(eps))
            stats.append((mean, alpha))
        idx += n
        log_q = log_q - ld
    return z, log_q, stats


def real_mask(D):
    return torch.tensor(embed_features(np.ones(D), D) > 0)


def padded_flow_forward(omega, params, D, S, L, U, eps, oracle):
    """The embedded chain -> (z (M, N, D), log_q, [(mean (D,), alpha (D,))], z_embedded (M, N, 2H)).  The base density is
    that of the real draw; every layer's log-det is taken at width 2H (the padded s are 0, the padded Affine alphas 0)."""
    W = 2 * half(D)
    real = real_mask(D)
    pe = torch.stack([torch.tensor(embed_row(row, D, S, L, U, oracle)) for row in params.detach().numpy()])
    z = torch.tensor(embed_features(np.asarray(omega), D)).to(torch.get_default_dtype())
    log_q = torch.tensor(oracle.base_log_density_f64(omega))
    idx, stats = 0, []
    for kind, n, upper in oracle.flow_layout(W, S, L, U):
        if kind == "coupling":
            z, ld = oracle.coupling(z, pe[:, idx:idx + n], W, L, U, upper, False)
        elif kind == "affine":
            z, ld = oracle.affine(z, pe[:, idx:idx + n], W, False)
        else:
            zn, ld, mean, alpha = oracle.bn_forward_batch(z[..., real].contiguous(), eps=oracle_eps(eps))
            z = z.clone()
            z[..., real] = zn  # the padded columns are left as they are: mean 0, alpha 1
            stats.append((mean, alpha))
        idx += n
        log_q = log_q - ld
    return z[..., real], log_q, stats, z
