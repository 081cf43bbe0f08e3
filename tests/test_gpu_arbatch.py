"""Sampling an autoregressive flow with fresh batch statistics as one C call each way (csrc/ar_flow_batch.hip,
include/tnf_arbatch.h; switch `NormFlow.ar_batch_forward`, families `ar_batch_chain` / `ar_batch_train`) on the GPU:
the reference's own nf(N) (tests/golden/maf.npz), forward values and gradients against the float64 restatement
(tests/arbatch_restatement.py, tied to float64 autograd by tests/test_arbatch_host.py), the contracts of the header, and
efn.train_efn end to end.

Every gradient error is max |got - want| / max |want| (conftest.grad_err) over the parameter row, as
tests/test_gpu_arsample.py takes it (each block's is printed beside it: arbatch_restatement.problem says where they part),
measured for the new route AND for the switch-off route (the per-bijector composition) on the same inputs.  The bar of a
shape is 4 x the larger of the switch-off route's error and the float32 noise of the folded restatement, never above
CAP = 2e-4 (tests/test_gpu_arsample.py); no bar comes from the new kernels' output.  The forward values are held to the
sampling-direction tolerance of test_maf_mfma_vs_oracle.  Recorded errors: profiles/r18_arbatch_grad_errors.json."""
import numpy as np
import pytest
import torch

from conftest import grad_err, load_golden
import arbatch_restatement as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available()
    return torch_nf_amd


def counts():
    from torch_nf_amd import _lib, arbatch_ops

    return ([arbatch_ops.arbatch_launch_count(w) for w in range(4)],
            int(_lib.lib.tnf_diag_launch_count(_lib.DIAG_MAF_BWD_MFMA)))


def delta(c0, c1):
    return [b - a for a, b in zip(c0[0], c1[0])], c1[1] - c0[1]


def fwd_tol(D):
    """test_maf_mfma_vs_oracle, sampling direction: the nets are iterated D - 1 times."""
    return dict(rtol=1e-4 * max(1, D // 8), atol=1e-4 * max(1, D // 8))


def make_flow(tnf, shape, pr, on, conditioner=True):
    D, L, U = shape[:3]
    np.random.seed(0)
    nf = tnf.NormFlow(D, conditioner, "AR", 1, L, U)
    nf.bijectors[0].set_masks(pr["ms"])
    nf.ar_batch_forward = on
    return nf


def base64(pr):
    return torch.tensor(B._oracle().base_log_density_f64(pr["omega"].double().numpy()))


def run(tnf, shape, pr, on, cz, cl):
    """One forward and backward of loss = cz sum(z w_z) + cl sum(log_q w_l) -> (g_params, z, log_q, mean, alpha)."""
    from torch_nf_amd import arbatch_ops, ops

    nf = make_flow(tnf, shape, pr, on)
    p = pr["params"].cuda().requires_grad_()
    omega = pr["omega"].cuda()
    if on and shape[3] != shape[4]:
        # one shared row under several blocks of draws: NormFlow offers the families to one block per row only (its own
        # draws are), so this layout of the header is reached through the autograd entry, as _forward_from calls it
        assert nf._route("forward", omega, p, freeze_bn=False).family == "bijectors"
        bn = nf.bijectors[1]
        z, sld, mean, alpha = arbatch_ops.ar_flow_forward_batch_train(omega, p, nf.bijectors[0]._masks_for(torch.float32),
                                                                      *shape[:3], bn.eps)
        bn.set_last_stats(mean, alpha)
        lq = ops.base_log_density_f64(omega) - sld
    else:
        z, lq = nf._forward_from(omega, p, freeze_bn=False)
    (cz * (z * pr["wz"].cuda()).sum() + cl * (lq * pr["wl"].cuda().double()).sum()).backward()
    bn = nf.bijectors[1]
    return p.grad, z.detach(), lq.detach(), bn.get_last_mean().detach(), bn.get_last_alpha().detach()


def check_forward(shape, pr, z, lq, mean, alpha, tag):
    tol = fwd_tol(shape[0])
    torch.testing.assert_close(z.cpu().double(), pr["z64"], **tol, msg=lambda m: tag + " z: " + m)
    torch.testing.assert_close(lq.cpu().double(), base64(pr) - pr["sld64"], **tol, msg=lambda m: tag + " log_q: " + m)
    torch.testing.assert_close(mean.cpu().double(), pr["mean64"], **tol, msg=lambda m: tag + " mean: " + m)
    torch.testing.assert_close(alpha.cpu().double(), pr["alpha64"], **tol, msg=lambda m: tag + " alpha: " + m)


def check_grads(tag, n, g_on, g_off, want, noise):
    """Print every figure (the whole row's, and each block's for the record), then hold the new route's gradient to its
    bar: 4 x the larger of the switch-off route's error and the folded restatement's float32 noise, at most CAP."""
    e_off = grad_err(tag + " switch off", g_off, want) if g_off is not None else 0.0
    e_on = grad_err(tag, g_on, want)
    bar = min(4.0 * max(e_off, noise), B.CAP)
    blocks = B.split_err(g_on, want, n) + (B.split_err(g_off, want, n) if g_off is not None else (0.0, 0.0))
    print("%s: on %.3e off %.3e noise %.3e bar %.3e | MAF block on %.3e off %.3e, Affine slice on %.3e off %.3e"
          % (tag, e_on, e_off, noise, bar, blocks[0], blocks[2], blocks[1], blocks[3]))
    assert e_on <= bar, "%s: gradient error %.3e of the largest entry exceeds %.1e" % (tag, e_on, bar)


# ---- the reference's own nf(N) ----------------------------------------------------------------------------------------------
def test_golden(tnf, monkeypatch):
    from torch_nf_amd import ops

    def no_bn_batch(*a, **k):
        raise AssertionError("the per-bijector batch-statistics BatchNorm ran")

    g = load_golden("maf")
    T = lambda a: torch.tensor(np.asarray(a)).float().cuda()  # noqa: E731
    for ci, (D, L, U, N) in enumerate(g["flow_meta"].tolist()):
        k = "n%02d_" % ci
        np.random.seed(0)
        nf = tnf.NormFlow(D, False, "AR", 1, L, U)
        nf.bijectors[0].set_masks([g[k + "ms%d" % i] for i in range(L + 1)])
        nf.params = T(g[k + "params"])
        nf.ar_batch_forward = True
        for grad in (False, True):
            nf.bijectors[1].set_last_stats(torch.zeros(D), torch.ones(D))
            p = nf.params.clone().requires_grad_(grad)
            assert nf._route("forward", T(g[k + "omega"]), p, freeze_bn=False).family == ("ar_batch_train" if grad else "ar_batch_chain")
            c0 = counts()
            with monkeypatch.context() as mp:
                mp.setattr(ops, "bn_batch_forward", no_bn_batch)
                z, lq = nf._forward_from(g[k + "omega"], p, freeze_bn=False)
                if grad:
                    (lq.mean() + (z ** 2).mean()).backward()
            assert delta(c0, counts()) == ([1, 4, int(grad), 4 * int(grad)], 0)
            torch.testing.assert_close(z.detach().cpu(), T(g[k + "z_fwd"]).cpu(), rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(lq.detach().cpu(), torch.tensor(g[k + "logq_fwd"]).double(), rtol=1e-5, atol=1e-4)
            bn = nf.bijectors[1]  # the statistics are cached on the layer, without a graph
            assert not bn.get_last_mean().requires_grad and not bn.get_last_alpha().requires_grad
            torch.testing.assert_close(bn.get_last_mean().cpu(), T(g[k + "bn_mean"]).cpu().reshape(-1), rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(bn.get_last_alpha().cpu(), T(g[k + "bn_alpha"]).cpu().reshape(-1), rtol=1e-4, atol=1e-4)
            if grad:
                assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


# ---- forward and gradients against the float64 restatement ---------------------------------------------------------------
@pytest.mark.parametrize("shape", B.TRAIN_SHAPES, ids=B.shape_id)
def test_forward_and_gradients(tnf, shape):
    pr = B.problem(shape)
    D = shape[0]
    if shape[3] == shape[4]:
        nf = make_flow(tnf, shape, pr, True)
        assert nf._route("forward", pr["omega"].cuda(), pr["params"].cuda().requires_grad_(), freeze_bn=False).family == "ar_batch_train"
    for name, cz, cl in B.LOSSES:
        c0 = counts()
        g_off, z_off, lq_off, mean_off, alpha_off = run(tnf, shape, pr, False, cz, cl)
        c1 = counts()
        g_on, z_on, lq_on, mean_on, alpha_on = run(tnf, shape, pr, True, cz, cl)
        c2 = counts()
        assert delta(c0, c1) == ([0, 0, 0, 0], D + 1)  # the composition: D + 1 launches of the inverse-direction backward
        assert delta(c1, c2) == ([1, 4, 1, 4], 0)       # one call, four kernels, each way
        tag = "arbatch %s loss %s" % (B.shape_id(shape), name)
        check_forward(shape, pr, z_off, lq_off, mean_off, alpha_off, tag + " switch off")
        check_forward(shape, pr, z_on, lq_on, mean_on, alpha_on, tag)
        check_grads(tag, pr["n"], g_on.cpu(), g_off.cpu(), pr["want"][name], pr["noise"][name])


@pytest.mark.parametrize("shape", B.FORWARD_ONLY, ids=B.shape_id)
def test_forward_outside_the_backward_domain(tnf, shape):
    """D > 32: `ar_batch_chain` without autograd, the composition with it."""
    pr = B.problem(shape)
    nf = make_flow(tnf, shape, pr, True)
    p = pr["params"].cuda()
    assert nf._route("forward", pr["omega"].cuda(), p, freeze_bn=False).family == "ar_batch_chain"
    assert nf._route("forward", pr["omega"].cuda(), p.clone().requires_grad_(), freeze_bn=False).family == "bijectors"
    c0 = counts()
    with torch.no_grad():
        z, lq = nf._forward_from(pr["omega"].cuda(), p, freeze_bn=False)
    assert delta(c0, counts()) == ([1, 4, 0, 0], 0)
    bn = nf.bijectors[1]
    check_forward(shape, pr, z, lq, bn.get_last_mean(), bn.get_last_alpha(), "arbatch %s" % B.shape_id(shape))


# ---- the entries themselves: contracts of the header -----------------------------------------------------------------------
def raw(tnf, shape, pr, g_z, g_sld, fill=0.0, offset=0):
    """One ctypes call of each entry on fresh buffers -> (z, sld, mean, alpha, g_params, backward workspace).  `offset`:
    omega, z and g_z start that many floats past a 16-byte boundary."""
    from torch_nf_amd import _lib

    lib, check = _lib.lib, _lib.check
    D, L, U, M, Mp, N = shape
    nf = make_flow(tnf, shape, pr, True)
    mk = nf.bijectors[0]._masks_for(torch.float32)

    def shifted(t):
        buf = torch.empty(t.numel() + 4, device="cuda")
        assert buf.data_ptr() % 16 == 0
        out = buf[offset:offset + t.numel()].view(t.shape)
        out.copy_(t)
        return out

    omega, p = shifted(pr["omega"].cuda()), pr["params"].cuda()
    P = p.shape[1]
    z = shifted(torch.zeros(M, N, D))
    sld, mean, alpha = torch.empty(M, N, device="cuda"), torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    nb = check(lib.tnf_ar_flow_forward_batch_workspace_bytes(M, Mp, N, D))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()
    check(lib.tnf_ar_flow_forward_batch_f32(omega.data_ptr(), p.data_ptr(), mk.data_ptr(), z.data_ptr(), sld.data_ptr(),
                                            mean.data_ptr(), alpha.data_ptr(), M, Mp, N, D, L, U, P, B.EPS, ws.data_ptr(), nb, st))
    gz = None if g_z is None else shifted(g_z.cuda())
    gs = None if g_sld is None else g_sld.cuda()
    gp = torch.full((Mp, P), fill, device="cuda")
    nb = check(lib.tnf_ar_flow_batch_bwd_workspace_bytes(M, Mp, N, D))
    wsb = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    check(lib.tnf_ar_flow_batch_bwd_f32(z.data_ptr(), p.data_ptr(), mk.data_ptr(), mean.data_ptr(), alpha.data_ptr(),
                                        None if gz is None else gz.data_ptr(), None if gs is None else gs.data_ptr(),
                                        gp.data_ptr(), M, Mp, N, D, L, U, P, P, wsb.data_ptr(), nb, st))
    torch.cuda.synchronize()
    return z, sld, mean, alpha, gp.cpu(), wsb.cpu()


def global_sums(shape, wsb):
    """P (D) | Q (D) | G out of the backward's workspace (ar_batch_bwd_ws of csrc/ar_flow_batch.hip: the partial sums of
    M BX slices, 2 D + 1 doubles each, then the global sums)."""
    D, _, _, M, _, N = shape
    rpi = 256 // D
    bx = max(1, min((N + 16 * rpi - 1) // (16 * rpi), max(1, 1024 // M)))
    off = M * bx * (2 * D + 1) * 8
    return torch.frombuffer(bytearray(wsb.numpy().tobytes()), dtype=torch.float64, count=2 * D + 1, offset=off).clone()


@pytest.mark.parametrize("shape", [B.TRAIN_SHAPES[0], B.TRAIN_SHAPES[1], B.TRAIN_SHAPES[12]], ids=B.shape_id)
def test_sums_are_bit_reproducible(tnf, shape):
    """P, Q, G (no atomics anywhere in their reduction) and, with per-context rows, the Affine slice: bit-equal over two
    calls.  The sums are also the restatement's, which pins the workspace layout this test reads them from."""
    pr = B.problem(shape)
    D, _, _, M, Mp, N = shape
    n = pr["n"]
    a = raw(tnf, shape, pr, pr["wz"], -pr["wl"])
    b = raw(tnf, shape, pr, pr["wz"], -pr["wl"])
    sa, sb = global_sums(shape, a[5]), global_sums(shape, b[5])
    assert torch.equal(a[0], b[0]) and torch.equal(sa, sb)
    if Mp == M:
        assert torch.equal(a[4][:, n:], b[4][:, n:])
    z, gz, gs = a[0].cpu().double(), pr["wz"].double(), -pr["wl"].double()
    aff, sh = pr["params"][:, None, n:n + D].double(), pr["params"][:, None, n + D:].double()
    want = torch.cat([(gz * torch.exp(aff)).sum((0, 1)), (gz * (z - sh)).sum((0, 1)), gs.sum().reshape(1)])
    torch.testing.assert_close(sa, want, rtol=1e-9, atol=1e-9 * float(want.abs().max()))


def test_prefilled_g_params(tnf):
    """include/tnf_arbatch.h with per-context rows: the MAF block is WRITTEN (a prefill of 1.0 leaves no trace, bit for
    bit), the Affine slice is ADDED to (1 + the gradient); callers zero g_params in every case."""
    shape = B.TRAIN_SHAPES[2]  # four private accumulator copies: bit-reproducible
    pr = B.problem(shape)
    n = pr["n"]
    zero = raw(tnf, shape, pr, pr["wz"], -pr["wl"], fill=0.0)[4]
    one = raw(tnf, shape, pr, pr["wz"], -pr["wl"], fill=1.0)[4]
    assert torch.equal(zero[:, :n], one[:, :n])
    torch.testing.assert_close(one[:, n:], 1.0 + zero[:, n:], rtol=2e-7, atol=2e-7)
    check_grads("arbatch prefilled %s" % B.shape_id(shape), n, zero, None, pr["want"]["both"], pr["noise"]["both"])


@pytest.mark.parametrize("name", ["both", "z", "log_q"])
def test_unaligned_rows_and_absent_cotangents(tnf, name):
    """omega, z and g_z one float past a 16-byte boundary at D = 16: the scalar-access instantiations of the apply pass and
    of the walk, by the launchers' predicates; the absent cotangent as NULL.  Forward values and gradients hold the bars
    of the aligned call."""
    shape = B.TRAIN_SHAPES[2]
    pr = B.problem(shape)
    g_z = None if name == "log_q" else pr["wz"]
    g_sld = None if name == "z" else -pr["wl"]
    z, sld, mean, alpha, gp, _ = raw(tnf, shape, pr, g_z, g_sld, offset=1)
    assert z.data_ptr() % 16 == 4
    check_forward(shape, pr, z, base64(pr).cuda() - sld.double(), mean, alpha, "arbatch unaligned")
    check_grads("arbatch unaligned %s loss %s" % (B.shape_id(shape), name), pr["n"], gp, None, pr["want"][name], pr["noise"][name])


def test_support_layer_and_cde(tnf):
    """cde(x, N) with a ToSimplex layer behind the family, per-context rows from a param_net: gradients reach every
    param_net parameter and equal the switch-off route's within the cap."""
    D, L, U, M, N, Dx = 4, 2, 15, 4, 16, 3
    torch.manual_seed(5)
    np.random.seed(5)
    nf = tnf.NormFlow(D, True, "AR", 1, L, U, support_layer=tnf.ToSimplex(D))
    cde = tnf.ConditionalDensityEstimator(nf, Dx, [16])
    cde.cuda()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, Dx, generator=g)
    wz, wl = torch.randn(M, N, D + 1, generator=g), torch.randn(M, N, generator=g)
    grads = {}
    for on in (False, True):
        nf.ar_batch_forward = on
        cde.param_net.zero_grad()
        np.random.seed(11)
        c0 = counts()
        z, log_q = cde(x.cuda(), N=N)
        ((z * wz.cuda()).sum() + (log_q * wl.cuda()).sum()).backward()
        assert delta(c0, counts()) == (([1, 4, 1, 4], 0) if on else ([0, 0, 0, 0], D + 1))
        grads[on] = [q.grad.clone() for q in cde.param_net.parameters()]
    for (pname, _), a, b in zip(cde.param_net.named_parameters(), grads[True], grads[False]):
        assert float(a.abs().max()) > 0
        tag = "arbatch through the CDE: d " + pname
        print(tag, "%.3e" % grad_err(tag, a, b))
        grad_err(tag, a, b, B.CAP)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_train_efn_through_the_captured_graph(tnf):
    from torch_nf_amd.efn import train_efn
    from torch_nf_amd.exponential_families import Dirichlet

    fam = Dirichlet(5)
    losses = {}
    for on in (False, True):
        torch.manual_seed(5)
        np.random.seed(5)
        nf = tnf.NormFlow(4, True, "AR", 1, 2, 15, support_layer=tnf.ToSimplex(4))
        nf.ar_batch_forward = on
        cde = tnf.ConditionalDensityEstimator(nf, fam.D_eta, [16])
        cde.cuda()
        torch.manual_seed(7)
        c0 = counts()
        losses[on], KLs = train_efn(cde, fam, M=8, N=16, num_iters=8, lr=1e-3, seed=3, use_graph=True)
        d = delta(c0, counts())[0]
        assert losses[on].shape == (8,) and np.isfinite(losses[on]).all() and np.isfinite(KLs).all()
        # three eager warm-up iterations and the capture call the entries; the four replays do not
        assert d == ([4, 16, 4, 16] if on else [0, 0, 0, 0])
    print("arbatch train_efn first losses: on %.6f off %.6f" % (losses[True][0], losses[False][0]))
    torch.testing.assert_close(torch.tensor(losses[True][0]), torch.tensor(losses[False][0]), **fwd_tol(4))
