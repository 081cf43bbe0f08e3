"""A torch float64 restatement of the walk of flow_sample_bwd_kernel (include/tnf_sampletrain.h): the backward of
frozen-statistics sampling from its output.  No autograd: from (z, G = d loss / d z, gamma = d loss / d sum_log_det) the
layers are met last to first, c = 2S-1 .. 0; each step puts the constant fold behind layer c back (x = A v + B, g <- g/A,
on odd c the fold gradients dA, dB and from them the Affine block's [alpha | shift] gradient) and then runs the coupling
layer backwards with its input rebuilt, x2 = (v2 - t) e^-s, d_t = g2, d_s = g2 (v2 - t) + gamma, g2 <- g2 e^s.  The state
the walk ends on is the base draw omega."""
import torch


def _dims(D, upper):
    h = D // 2
    return (h, D - h) if upper else (D - h, h)


def _layer_back(v, g, gamma, p, D, L, U, upper):
    """One coupling layer of the walk on the (M, N, D) state v (the layer's OUTPUT) and gradient g, log-det cotangent
    gamma (M, N), parameter block p (M, n) -> (the layer's input, the gradient w.r.t. it, g_p (M, n))."""
    M = v.shape[0]
    h = D // 2
    din, dout = _dims(D, upper)
    cs, ts = (slice(0, h), slice(h, D)) if upper else (slice(h, D), slice(0, h))
    x, v2, g1, g2 = v[:, :, cs], v[:, :, ts], g[:, :, cs], g[:, :, ts]
    W, off = [], 0
    for i, o in [(din, U)] + [(U, U)] * (L - 1) + [(U, dout)]:
        wt = p[:, off:off + i * o].view(M, i, o)
        ws = p[:, off + i * o:off + 2 * i * o].view(M, i, o)
        bt = p[:, off + 2 * i * o:off + 2 * i * o + o].view(M, 1, o)
        bs = p[:, off + 2 * i * o + o:off + 2 * i * o + 2 * o].view(M, 1, o)
        W.append((off, i, o, (wt, ws), (bt, bs)))
        off += 2 * i * o + 2 * o
    acts, out = [[x], [x]], [None, None]
    for net in range(2):  # (t, s) recomputed from the conditioner half, which the layer leaves unchanged
        a = x
        for li, (_, i, o, w, b) in enumerate(W):
            a = torch.matmul(a, w[net]) + b[net]
            if li < L:
                a = torch.tanh(a)
                acts[net].append(a)
        out[net] = a
    t, s = out
    d = v2 - t
    x2 = d * torch.exp(-s)
    delta = [g2, g2 * d + gamma[:, :, None]]
    g2_in = g2 * torch.exp(s)
    gp = torch.zeros_like(p)
    dx = torch.zeros_like(x)
    for net in range(2):
        dl = delta[net]
        for li in range(L, -1, -1):
            off, i, o, w, _ = W[li]
            a_in = acts[net][li]
            gp[:, off + net * i * o:off + (net + 1) * i * o] = torch.einsum("mni,mno->mio", a_in, dl).reshape(M, i * o)
            gp[:, off + 2 * i * o + net * o:off + 2 * i * o + (net + 1) * o] = dl.sum(1)
            dl = torch.matmul(dl, w[net].transpose(1, 2))
            if li > 0:
                dl = dl * (1.0 - a_in * a_in)
        dx = dx + dl
    v_in, g_in = torch.empty_like(v), torch.empty_like(g)
    v_in[:, :, cs], v_in[:, :, ts] = x, x2
    g_in[:, :, cs], g_in[:, :, ts] = g1 + dx, g2_in
    return v_in, g_in, gp


def sample_bwd(z, params, mean, alpha, G, gamma, D, S, L, U):
    """(omega (M, N, D), g_params (M_p, P)) float64 from the sampling output z (M, N, D), params (M_p, >= P) with M_p in
    {1, M}, the frozen statistics mean / alpha (2S, D) and the two cotangents G (M, N, D) and gamma (M, N)."""
    M = z.shape[0]
    z, params, mean, alpha, G, gamma = (t.double() for t in (z, params, mean, alpha, G, gamma))
    Mp = params.shape[0]
    p = params.expand(M, params.shape[1])
    h = D // 2
    p_up = 2 * (h * U + (D - h) * U + (D - h) + U + (L - 1) * (U + 1) * U)
    p_low = 2 * ((D - h) * U + h * U + h + U + (L - 1) * (U + 1) * U)
    stage = p_up + p_low + 2 * D
    gp = torch.zeros(M, stage * S, dtype=torch.float64)
    v, g = z, G
    for c in range(2 * S - 1, -1, -1):
        b = (c >> 1) * stage
        A, B = alpha[c].expand(M, 1, D), mean[c].expand(M, 1, D)
        if c & 1:  # BatchNorm and the Affine y = e^a x + shift behind the layer: y = (x - B)/A
            a, shift = p[:, None, b + p_up + p_low:b + p_up + p_low + D], p[:, None, b + p_up + p_low + D:b + stage]
            A = alpha[c] / torch.exp(a)
            B = mean[c] - shift * A
        y = v
        v = A * y + B
        g = g / A
        if c & 1:
            dA, dB = -(g * y).sum(1, keepdim=True), -g.sum(1, keepdim=True)
            gp[:, b + p_up + p_low:b + p_up + p_low + D] = (-A * dA + shift * A * dB)[:, 0] + gamma.sum(1)[:, None]
            gp[:, b + p_up + p_low + D:b + stage] = (-A * dB)[:, 0]
        upper = (c & 1) == 0
        lo, n = (b, p_up) if upper else (b + p_up, p_low)
        v, g, gp[:, lo:lo + n] = _layer_back(v, g, gamma, p[:, lo:lo + n], D, L, U, upper)
    return v, (gp.sum(0, keepdim=True) if Mp == 1 else gp)
