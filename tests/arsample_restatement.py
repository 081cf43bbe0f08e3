"""The algorithm of maf_sample_bwd_kernel (csrc/maf_sample_bwd.hip) restated in torch, dtype-generic and without
autograd: one evaluation of the twin masked MLPs at the sample, D - 1 delta-only sweeps, one last pass with the weight
gradients, and (AR-stack mode) the fold in the load stage with its three sums.  tests/test_arsample_host.py holds it to
float64 autograd through the oracle."""
import torch


def _weights(params, D, L, U, Ms):
    """[(W_mu, W_alpha)] per layer, masked, (M_p, in, out)."""
    dims, off, out = [D] + [U] * L + [D], 0, []
    for i in range(L + 1):
        n = dims[i] * dims[i + 1]
        mask = torch.as_tensor(Ms[i], dtype=params.dtype)[None]
        pair = []
        for _ in range(2):
            pair.append(mask * params[:, off:off + n].reshape(-1, dims[i], dims[i + 1]))
            off += n
        out.append(pair)
    return out


def _evaluate(x, W):
    """-> (inputs of every layer per net, mu, alpha)."""
    acts, outs = [[x], [x]], []
    for net in range(2):
        h = x
        for i, w in enumerate(W):
            a = torch.matmul(h, w[net])
            if i < len(W) - 1:
                h = torch.tanh(a)
                acts[net].append(h)
            else:
                outs.append(a)
    return acts, outs[0], outs[1]


def _back(d_mu, d_alpha, acts, W, want_w):
    """Deltas back through layers L .. 0 -> (the nets' gradient w.r.t. x, [per layer (dW_mu, dW_alpha)] or None)."""
    nx, gw = 0.0, [[None, None] for _ in W]
    for net, d in ((0, d_mu), (1, d_alpha)):
        for i in range(len(W) - 1, -1, -1):
            inp = acts[net][i]
            if want_w:
                gw[i][net] = torch.matmul(inp.transpose(1, 2), d)
            d = torch.matmul(d, W[i][net].transpose(1, 2))
            if i > 0:
                d = d * (1.0 - inp ** 2)  # tanh' = 4 r (1 - r)
        nx = nx + d
    return nx, (gw if want_w else None)


def maf_sample_bwd(x, params, Ms, g_x, g_ld, D, L, U, sweeps=None):
    """x (M, N, D) the sample, params (M_p, P), cotangents g_x (M, N, D) and g_ld (M, N)
    -> (g_omega, g_params (M_p, P), [v after each sweep])."""
    W = _weights(params, D, L, U, Ms)
    acts, mu, alpha = _evaluate(x, W)
    e, ea, xm = torch.exp(-alpha), torch.exp(alpha), x - mu

    def deltas(v):
        ve = v * e
        return -ve, -ve * xm - g_ld[:, :, None]

    v, trail = ea * g_x, []
    for _ in range(D - 1 if sweeps is None else sweeps):
        nv, _ = _back(*deltas(v), acts, W, False)
        v = ea * (g_x - nv)
        trail.append(v)
    _, gw = _back(*deltas(v), acts, W, True)
    rows = []
    for i, pair in enumerate(gw):
        mask = torch.as_tensor(Ms[i], dtype=params.dtype)[None]
        for g in pair:
            g = -(g * mask)  # g_theta = -K_theta, negated at the flush
            if params.shape[0] == 1:
                g = g.sum(0, keepdim=True)
            rows.append(g.reshape(g.shape[0], -1))
    return v, torch.cat(rows, 1), trail


def ar_flow_sample_bwd(z, params, Ms, bn_mean, bn_alpha, g_z, g_sld, D, L, U):
    """The AR-stack mode: z (M, N, D) the stack's output, params (M_p, P_maf + 2 D) = [MAF | a | b]
    -> g_params (M_p, P_maf + 2 D)."""
    n = params.shape[1] - 2 * D
    a, b = params[:, n:n + D], params[:, n + D:]
    A = bn_alpha[None] * torch.exp(-a)
    B = bn_mean[None] - b * A
    x = z * A[:, None] + B[:, None]
    _, g_maf, _ = maf_sample_bwd(x, params[:, :n], Ms, g_z / A[:, None], g_sld, D, L, U)
    GZ, GB, GS = (g_z * z).sum(1), g_z.sum(1), g_sld.sum(1)
    if params.shape[0] == 1:
        GZ, GB, GS = GZ.sum(0, keepdim=True), GB.sum(0, keepdim=True), GS.sum(0, keepdim=True)
    return torch.cat([g_maf, GZ - b * GB + GS[:, None], GB], 1)
