#!/usr/bin/env python3
"""Sampling with fresh batch statistics (NormFlow.forward with freeze_bn=False: the reference's default sampling
call and, under autograd, its train_efn loop, notebooks/two_network_arch.ipynb:84-92) at D=64, 8 coupling layers:
the one-call chains (tnf_flow_forward_batch_f32, tnf_flow_forward_train_fwd/bwd_f32) against the per-bijector
composition, and an EFN-style step with Adam eagerly and as one HIP graph.  Then the real thing: the EFN loss
mean(log_q - eta . T(z)) of exponential_families.efn_loss (fused kernel tnf_ef_dot) alone and inside the training step,
against the materialised formulation it replaces (T(z) then torch.matmul).  Usage: python tools/efnbench.py"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402


def bench(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


D, S, L, U = 64, 4, 2, 15
nf = tnf.NormFlow(D, False, "coupling", S, L, U)
nf.params = (torch.randn(1, nf.D_params) * 0.1).cuda().requires_grad_()
for N in (1 << 16, 1 << 19):
    omega = torch.randn(1, N, D, device="cuda")

    def sample():
        with torch.no_grad():
            nf._forward_from(omega, nf.params, freeze_bn=False)

    def train():
        nf.params.grad = None
        z, lq = nf._forward_from(omega, nf.params, freeze_bn=False)
        (lq.mean() + (z ** 2).mean()).backward()

    def frozen():
        with torch.no_grad():
            nf._forward_from(omega, nf.params, freeze_bn=True)

    row = []
    for fused in (True, False):
        nf.fused_batch_forward = fused
        row.append((bench(sample), bench(train)))
    nf.fused_batch_forward = True
    print("N=%7d  fresh statistics, no autograd: %.3f ms (per bijector %.3f)   with backward: %.3f ms (per bijector %.3f)"
          "   frozen statistics: %.3f ms" % (N, row[0][0], row[1][0], row[0][1], row[1][1], bench(frozen)))

opt = torch.optim.Adam([nf.params], lr=1e-4, capturable=True)
for N in (1 << 14, 1 << 16):
    def step():
        opt.zero_grad(set_to_none=True)
        z, lq = nf.sample(N, freeze_bn=False)
        loss = lq.mean() + (z ** 2).mean()
        loss.backward()
        opt.step()
        return loss.detach()

    te = bench(step)
    gs = tnf.graphs.GraphedStep(step, warmup=3)
    print("N=%7d  EFN-style step (device draw, fresh statistics, backward, Adam): eager %.3f ms, one HIP graph %.3f ms"
          % (N, te, bench(gs)))


# ---- the EFN loss itself: fused eta . T(z) against the materialised formulation -------------------------------------
from torch_nf_amd.exponential_families import MVN, efn_loss  # noqa: E402

HBM = 8.0e12  # B/s, the MI355X's nominal HBM3E bandwidth: the roof the fractions below refer to


def spread(fn, reps=20):
    """median and (min, max) in ms over `reps` timed calls after a settling run of ~0.2 s"""
    t_end = time.perf_counter() + 0.2
    while time.perf_counter() < t_end:
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def T_pure(z):  # the reference's MVN.T in torch ops (outer product, gather of the upper triangle, concatenate)
    r, c = torch.triu_indices(z.shape[2], z.shape[2], device=z.device)
    return torch.cat((z, (z[:, :, :, None] * z[:, :, None, :])[:, :, r, c]), dim=2)


print("\nloss term eta . T(z), MVN, float32: median ms (min .. max of 20)")
for M, N, Dd in ((1, 1 << 19, 64), (64, 1 << 14, 64), (1024, 1024, 20), (100, 100, 5)):
    fam = MVN(Dd)
    eta = (torch.randn(M, fam.D_eta, device="cuda") * 0.1)
    Nm = N
    while M * Nm * fam.D_eta * 4 * 3 > 24e9:  # the materialised rows keep T(z), the outer product and its gradient
        Nm //= 2
    for label, n in (("fused", N), ("materialised", Nm)):
        z = torch.randn(M, n, Dd, device="cuda")
        zg = z.clone().requires_grad_()
        lq = torch.randn(M, n, device="cuda")
        rows = {}
        if label == "fused":
            rows["fused fwd"] = lambda: fam.eta_dot_T(z, eta)
            rows["fused fwd+bwd"] = lambda: torch.autograd.grad(efn_loss(zg, lq, eta, fam), zg)
        else:
            rows["T kernel + matmul fwd"] = lambda: torch.matmul(fam.T(z), eta[:, :, None])
            rows["T kernel + matmul fwd+bwd"] = lambda: torch.autograd.grad(
                torch.mean(lq - torch.matmul(fam.T(zg), eta[:, :, None])[:, :, 0]), zg)
            rows["pure torch fwd"] = lambda: torch.matmul(T_pure(z), eta[:, :, None])
            rows["pure torch fwd+bwd"] = lambda: torch.autograd.grad(
                torch.mean(lq - torch.matmul(T_pure(zg), eta[:, :, None])[:, :, 0]), zg)
        for name, fn in rows.items():
            med, lo, hi = spread(fn)
            byts = 4 * (Dd + 1) if name.endswith("fwd") else 4 * (3 * Dd + 3)  # fwd+bwd: z twice, g_z, out, g_out
            extra = "  %5.1f %% of the HBM roof at %d B/sample" % (100 * M * n * byts / (med * 1e-3) / HBM, byts) \
                if label == "fused" else ""
            print("(M,N,D)=(%d,%d,%d)%s %-26s %9.4f ms (%.4f .. %.4f)  %8.1f M samples/s%s"
                  % (M, n, Dd, "" if n == N else " [N cut to fit]", name, med, lo, hi, M * n / med / 1e3, extra))
        del z, zg, lq
        torch.cuda.empty_cache()

print("\ntrue EFN step: MVN(64), NormFlow(64, False, 'coupling', 4, 2, 15), device draw, fresh statistics, efn_loss, "
      "backward, Adam")
fam = MVN(64)
eta1 = torch.randn(1, fam.D_eta, device="cuda") * 0.05
for N in (1 << 14, 1 << 16, 1 << 19):
    def efn_step():
        opt.zero_grad(set_to_none=True)
        z, lq = nf.sample(N, freeze_bn=False)
        loss = efn_loss(z, lq, eta1, fam)
        loss.backward()
        opt.step()
        return loss.detach()

    with torch.no_grad():
        zs, lqs = nf.sample(N, freeze_bn=False)
    zs = zs.detach().requires_grad_()
    t_loss = spread(lambda: torch.autograd.grad(efn_loss(zs, lqs, eta1, fam), zs))[0]
    te = spread(efn_step)
    gs = tnf.graphs.GraphedStep(efn_step, warmup=3)
    tg = spread(gs)
    print("N=%7d  eager %.3f ms (%.3f .. %.3f), one HIP graph %.3f ms (%.3f .. %.3f); loss forward+backward alone "
          "%.4f ms = %.1f %% of the graphed step" % ((N,) + te + tg + (t_loss, 100 * t_loss / tg[0])))
