"""A torch float32 restatement of the walk of csrc/flow_ctx_bwd.hip (include/tnf_ctxtrain.h): the backward of a
per-context coupling flow's log_prob from the z0 that the forward kept.  No autograd: explicit delta formulas, layer by
layer, the bijectors first to last, each coupling layer's input rebuilt by the sampling-direction map.

`pad_to`: the samples of a context are filled up to a multiple of `pad_to` rows with copies of the last row that carry
zero upstream gradient -- what a tiled kernel computes and never stores.  They must contribute exactly nothing: every
delta and every gradient entry of such a row is +-0 (`PAD_ABS` keeps the largest magnitude seen by the latest call), and
the sums over a context's samples run in the fixed order n = 0, 1, ... so that the zeros are added last.  The result is
cut back to N rows.  (The shipped kernel forms no such rows; the restatement pins that they would be harmless.)"""
import torch

PAD_ABS = [0.0]  # the largest |delta| or |gradient| on a row beyond N in the latest log_prob_bwd call


def _sum_samples(t):
    """Sum over dim 1 (the samples) in the order n = 0, 1, ...: the kernel's order."""
    acc = torch.zeros_like(t[:, 0])
    for n in range(t.shape[1]):
        acc = acc + t[:, n]
    return acc


def _note_pad(t, n_real):
    if t.shape[1] > n_real:
        PAD_ABS[0] = max(PAD_ABS[0], float(t[:, n_real:].abs().max()))


def _dims(D, upper):
    h = D // 2
    return (h, D - h) if upper else (D - h, h)


def _coupling_back(z, G, gl, p, D, L, U, upper, n_real):
    """One coupling layer of the walk on (M, N, D) state z and gradient G, log-det cotangent gl (M, N), parameter block
    p (M, n) -> (z', G', g_p (M, n))."""
    M = z.shape[0]
    h = D // 2
    din, dout = _dims(D, upper)
    cs, ts = (slice(0, h), slice(h, D)) if upper else (slice(h, D), slice(0, h))
    x, z2, G1, G2 = z[:, :, cs], z[:, :, ts], G[:, :, cs], G[:, :, ts]
    sizes = [(din, U)] + [(U, U)] * (L - 1) + [(U, dout)]
    # forward, keeping the activations: acts[net][l] is the input of layer l
    W, off = [], 0
    for i, o in sizes:
        wt = p[:, off:off + i * o].view(M, i, o)
        ws = p[:, off + i * o:off + 2 * i * o].view(M, i, o)
        bt = p[:, off + 2 * i * o:off + 2 * i * o + o].view(M, 1, o)
        bs = p[:, off + 2 * i * o + o:off + 2 * i * o + 2 * o].view(M, 1, o)
        W.append((off, i, o, (wt, ws), (bt, bs)))
        off += 2 * i * o + 2 * o
    acts = [[x], [x]]
    out = [None, None]
    for net in range(2):
        a = x
        for li, (_, i, o, w, b) in enumerate(W):
            a = torch.matmul(a, w[net]) + b[net]
            if li < L:
                a = torch.tanh(a)
                acts[net].append(a)
        out[net] = a
    t, s = out
    # the layer: log_prob ran z2 = (y2 - t) e^-s
    y2 = t + z2 * torch.exp(s)
    Gy = G2 * torch.exp(-s)
    delta = [-Gy, gl[:, :, None] - G2 * z2]
    gp = torch.zeros_like(p)
    dx = torch.zeros_like(x)
    for net in range(2):
        d = delta[net]
        for li in range(L, -1, -1):
            off, i, o, w, _ = W[li]
            a_in = acts[net][li]
            _note_pad(d, n_real)
            gw = _sum_samples(a_in[:, :, :, None] * d[:, :, None, :])  # sum over the context's samples
            gb = _sum_samples(d)
            gp[:, off + net * i * o:off + (net + 1) * i * o] = gw.reshape(M, i * o)
            gp[:, off + 2 * i * o + net * o:off + 2 * i * o + (net + 1) * o] = gb
            d = torch.matmul(d, w[net].transpose(1, 2))
            if li > 0:
                d = d * (1.0 - a_in * a_in)
        dx = dx + d
    z_new, G_new = torch.empty_like(z), torch.empty_like(G)
    z_new[:, :, cs], z_new[:, :, ts] = x, y2
    G_new[:, :, cs], G_new[:, :, ts] = G1 + dx, Gy
    return z_new, G_new, gp


def log_prob_bwd(z0, params, mean, alpha, g_lp, D, S, L, U, pad_to=16):
    """(g_params (M, P), g_z (M, N, D)) float32 from z0 (M, N, D), params (M, >= P), mean / alpha (2S, D), g_lp (M, N)."""
    M, N, _ = z0.shape
    z0, params, mean, alpha, g_lp = (t.float() for t in (z0, params, mean, alpha, g_lp))
    extra = (-N) % pad_to if pad_to else 0
    if extra:
        z0 = torch.cat([z0, z0[:, -1:].expand(M, extra, D)], dim=1)
        g_lp = torch.cat([g_lp, torch.zeros(M, extra)], dim=1)
    h = D // 2
    p_up = 2 * (h * U + (D - h) * U + (D - h) + U + (L - 1) * (U + 1) * U)
    p_low = 2 * ((D - h) * U + h * U + h + U + (L - 1) * (U + 1) * U)
    stage = p_up + p_low + 2 * D
    gp = torch.zeros(M, stage * S)
    z, G, gl = z0, -g_lp[:, :, None] * z0, -g_lp
    PAD_ABS[0] = 0.0
    for st in range(S):
        b = st * stage
        z, G, gp[:, b:b + p_up] = _coupling_back(z, G, gl, params[:, b:b + p_up], D, L, U, True, N)
        z, G = (z - mean[2 * st]) / alpha[2 * st], G * alpha[2 * st]
        b += p_up
        z, G, gp[:, b:b + p_low] = _coupling_back(z, G, gl, params[:, b:b + p_low], D, L, U, False, N)
        z, G = (z - mean[2 * st + 1]) / alpha[2 * st + 1], G * alpha[2 * st + 1]
        b += p_low
        a, shift = params[:, None, b:b + D], params[:, None, b + D:b + 2 * D]
        gp[:, b:b + D] = _sum_samples(gl[:, :, None] - G * z)
        G = G * torch.exp(-a)
        gp[:, b + D:b + 2 * D] = -_sum_samples(G)
        _note_pad(G, N)
        z = z * torch.exp(a) + shift
    return gp, G[:, :N].contiguous()
