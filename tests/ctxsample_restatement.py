"""A torch float32 restatement of the walk of csrc/flow_ctx_sample_bwd.hip (include/tnf_ctxsample.h): the backward of a
per-context coupling flow's frozen-statistics sampling pass from the z that the forward returned.  No autograd: explicit
delta formulas, layer by layer, the bijectors last to first, each layer's input rebuilt by the inverse map.  Per stage:
the Affine block, BatchNorm c1, the lower coupling layer, BatchNorm c0, the upper coupling layer.

`reference` is what the restatement and the kernel are both held against: float64 autograd through the composition of
oracle.flow_forward (the same bijector functions in the same order) on float64 copies of the inputs, with the draw as a
leaf so that its gradient exists too.  `upstream` draws the two cotangents."""
import torch


def _sum_samples(t):
    """Sum over dim 1 (the samples) in the order n = 0, 1, ...: the kernel's order."""
    acc = torch.zeros_like(t[:, 0])
    for n in range(t.shape[1]):
        acc = acc + t[:, n]
    return acc


def _coupling_back(y, G, gl, p, D, L, U, upper):
    """One coupling layer of the walk on (M, N, D) output y and its gradient G, log-det cotangent gl (M, N), parameter
    block p (M, n) -> (x, G(x), g_p (M, n))."""
    M = y.shape[0]
    h = D // 2
    din, dout = (h, D - h) if upper else (D - h, h)
    cs, ts = (slice(0, h), slice(h, D)) if upper else (slice(h, D), slice(0, h))
    x1, y2, G1, G2 = y[:, :, cs], y[:, :, ts], G[:, :, cs], G[:, :, ts]
    sizes = [(din, U)] + [(U, U)] * (L - 1) + [(U, dout)]
    W, off = [], 0
    for i, o in sizes:
        wt = p[:, off:off + i * o].view(M, i, o)
        ws = p[:, off + i * o:off + 2 * i * o].view(M, i, o)
        bt = p[:, off + 2 * i * o:off + 2 * i * o + o].view(M, 1, o)
        bs = p[:, off + 2 * i * o + o:off + 2 * i * o + 2 * o].view(M, 1, o)
        W.append((off, i, o, (wt, ws), (bt, bs)))
        off += 2 * i * o + 2 * o
    # the twin nets from the conditioner half, which the layer left unchanged; acts[net][l] is the input of layer l
    acts = [[x1], [x1]]
    out = [None, None]
    for net in range(2):
        a = x1
        for li, (_, i, o, w, b) in enumerate(W):
            a = torch.matmul(a, w[net]) + b[net]
            if li < L:
                a = torch.tanh(a)
                acts[net].append(a)
        out[net] = a
    t, s = out
    # the layer: sampling ran y2 = t + x2 e^s
    x2 = (y2 - t) * torch.exp(-s)
    Gx = G2 * torch.exp(s)
    delta = [G2, Gx * x2 + gl[:, :, None]]
    gp = torch.zeros_like(p)
    dx = torch.zeros_like(x1)
    for net in range(2):
        d = delta[net]
        for li in range(L, -1, -1):
            off, i, o, w, _ = W[li]
            a_in = acts[net][li]
            gw = _sum_samples(a_in[:, :, :, None] * d[:, :, None, :])  # sum over the context's samples
            gb = _sum_samples(d)
            gp[:, off + net * i * o:off + (net + 1) * i * o] = gw.reshape(M, i * o)
            gp[:, off + 2 * i * o + net * o:off + 2 * i * o + (net + 1) * o] = gb
            d = torch.matmul(d, w[net].transpose(1, 2))
            if li > 0:
                d = d * (1.0 - a_in * a_in)
        dx = dx + d
    x_new, G_new = torch.empty_like(y), torch.empty_like(G)
    x_new[:, :, cs], x_new[:, :, ts] = x1, x2
    G_new[:, :, cs], G_new[:, :, ts] = G1 + dx, Gx
    return x_new, G_new, gp


def sample_bwd(z, params, mean, alpha, g_z, g_sld, D, S, L, U):
    """(g_params (M, P), g_omega (M, N, D), omega rebuilt (M, N, D)) float32 from the forward's z (M, N, D), params
    (M, >= P), mean / alpha (2S, D) and the upstream gradients g_z (M, N, D) | None and g_sld (M, N) | None (None: zero)."""
    M, N, _ = z.shape
    z, params, mean, alpha = (t.float() for t in (z, params, mean, alpha))
    G = torch.zeros(M, N, D) if g_z is None else g_z.float()
    gl = torch.zeros(M, N) if g_sld is None else g_sld.float()
    h = D // 2
    p_up = 2 * (h * U + (D - h) * U + (D - h) + U + (L - 1) * (U + 1) * U)
    p_low = 2 * ((D - h) * U + h * U + h + U + (L - 1) * (U + 1) * U)
    stage = p_up + p_low + 2 * D
    gp = torch.zeros(M, stage * S)
    for st in range(S - 1, -1, -1):
        b = st * stage + p_up + p_low
        a, shift = params[:, None, b:b + D], params[:, None, b + D:b + 2 * D]
        gp[:, b + D:b + 2 * D] = _sum_samples(G)  # Affine: y = x e^a + shift
        z = (z - shift) * torch.exp(-a)
        G = G * torch.exp(a)
        gp[:, b:b + D] = _sum_samples(G * z + gl[:, :, None])
        z, G = z * alpha[2 * st + 1] + mean[2 * st + 1], G / alpha[2 * st + 1]  # BatchNorm c1: y = (x - mu) / alpha
        b = st * stage + p_up
        z, G, gp[:, b:b + p_low] = _coupling_back(z, G, gl, params[:, b:b + p_low], D, L, U, False)
        z, G = z * alpha[2 * st] + mean[2 * st], G / alpha[2 * st]  # BatchNorm c0
        b = st * stage
        z, G, gp[:, b:b + p_up] = _coupling_back(z, G, gl, params[:, b:b + p_up], D, L, U, True)
    return gp, G.contiguous(), z.contiguous()


def upstream(M, N, D, seed=0):
    """(g_z (M, N, D), g_sld (M, N)) ~ N(0, 1)."""
    g = torch.Generator().manual_seed(91 + 1000 * D + 100 * M + N + seed)
    return torch.randn(M, N, D, generator=g), torch.randn(M, N, generator=g)


def flow_forward64(oracle, omega64, p64, D, S, L, U, stats64):
    """(z, sum_log_det (M, N)) in float64: the composition of oracle.flow_forward (frozen statistics) on tensors, so that
    autograd reaches the draw as well as the parameters.  Run under domain_helpers.float64()."""
    z, sld, idx, bn_i = omega64, torch.zeros(omega64.shape[:2], dtype=torch.float64), 0, 0
    for kind, n, upper in oracle.flow_layout(D, S, L, U):
        if kind == "coupling":
            z, ld = oracle.coupling(z, p64[:, idx:idx + n], D, L, U, upper, False)
            idx += n
        elif kind == "affine":
            z, ld = oracle.affine(z, p64[:, idx:idx + n], D, False)
            idx += n
        else:
            z, ld = oracle.bn_forward_frozen(z, *stats64[bn_i])
            bn_i += 1
        sld = sld + ld
    return z, sld


_REF = {}


def reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=None):
    """(g_params, g_omega) float64 of sum(z g_z) + sum(sum_log_det g_sld) (a None cotangent: that term absent); computed
    once per `key` and left unchanged."""
    if key is None or key not in _REF:
        D, S, L, U = shape
        with float64():
            P = oracle.flow_num_params(D, S, L, U)
            p64, o64 = params[:, :P].double().requires_grad_(), omega.double().requires_grad_()
            z, sld = flow_forward64(oracle, o64, p64, D, S, L, U, [(m.double(), a.double()) for m, a in zip(mean, alpha)])
            loss = 0.0
            if g_z is not None:
                loss = loss + (z * g_z.double()).sum()
            if g_sld is not None:
                loss = loss + (sld * g_sld.double()).sum()
            loss.backward()
        if key is None:
            return p64.grad, o64.grad
        _REF[key] = (p64.grad, o64.grad)
    return _REF[key]


def row_err(got, want):
    """The largest error of a context's row relative to that row's largest entry, over the contexts."""
    got, want = got.detach().double().cpu().flatten(1), want.detach().double().cpu().flatten(1)
    return float(((got - want).abs().max(1).values / want.abs().max(1).values.clamp_min(1e-300)).max())


# ---- the cases of tests/test_gpu_ctx_sample.py, shared with the CPU check of the restatement: (D, S, L, U, M, N) -------
WIDTHS_AND_SAMPLES = [(D, 2, 2, 15, 5, N) for D in (2, 5, 16, 31, 32, 33, 63, 64) for N in (1, 2, 15, 16, 17, 31)]
DEPTH_AND_UNITS = [(D, S, L, 16, 3, 7) for D in (5, 64) for L in (1, 3) for S in (1, 9)]
WORKGROUP_EDGES = [(6, 2, 2, 15, M, 3) for M in (1, 3, 4, 5)]
LARGEST_SLICE = [(64, 1, 3, 16, M, 31) for M in (1, 5)]
GRID = WIDTHS_AND_SAMPLES + DEPTH_AND_UNITS + WORKGROUP_EDGES + LARGEST_SLICE
