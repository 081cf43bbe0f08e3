"""Time a reparameterised step of an autoregressive flow -- z, log_q = nf(N) with frozen statistics under autograd, a loss
of both, backward (no optimiser) -- with NormFlow.ar_sample_training on (the one-kernel forward, the one fused backward
kernel of include/tnf_arsample.h) against the same flow with the switch off in the same process (the route such a call
takes otherwise: one kernel per bijector, and for the MAF tnf_maf_inverse_alpha, D + 1 backward launches and about 3 D
elementwise operations).

    python tools/arsamplebench.py [--n 262144] [--contexts 2000] [--reps 15] [--settle 5] [--out FILE.json]

Cells: (D, L, U) in (4, 2, 20), (6, 2, 15), (16, 2, 32), (21, 2, 42), (32, 2, 16); one shared parameter row with N = --n
samples, and the LFI layout, --contexts parameter rows x 100 samples.  Protocol: both variants are warmed up until the
clocks have settled (--settle steps), then timed in alternation, one step each per round, with device events; the figure
is the median of --reps rounds with the smallest and largest round beside it.  Prints one line per cell and writes
everything to --out as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402

CELLS = ((4, 2, 20), (6, 2, 15), (16, 2, 32), (21, 2, 42), (32, 2, 16))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, settle, reps):
    """{name: (median, min, max) ms} of the callables, timed in alternation after `settle` untimed rounds."""
    for _ in range(settle):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def cell(D, L, U, M, N, settle, reps):
    rng = np.random.RandomState(D)
    np.random.seed(D)
    fns, route = {}, None
    omega = torch.randn(M, N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(D))
    wz, wl = torch.randn_like(omega), torch.randn(M, N, device="cuda", dtype=torch.float64)
    for switch in (False, True):
        np.random.seed(D)
        nf = tnf.NormFlow(D, True, "AR", 1, L, U)
        nf.ar_sample_training = switch
        nf.bijectors[1].set_last_stats(torch.tensor(rng.normal(0, 0.1, D)).float().cuda(),
                                       torch.tensor(rng.uniform(0.8, 1.25, D)).float().cuda())
        p = torch.tensor(np.random.RandomState(D).normal(0, 0.2, (M, nf.D_params)), dtype=torch.float32,
                         device="cuda").requires_grad_()
        if switch:
            route = nf._route("forward", omega, p).family

        def step(nf=nf, p=p):
            z, lq = nf._forward_from(omega, p, freeze_bn=True)
            torch.autograd.grad((z * wz).sum() + (lq * wl).sum(), p)

        fns["on" if switch else "off"] = step
    return route, alternate(fns, settle, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--contexts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for layout, M, N in (("shared row", 1, a.n), ("LFI rows", a.contexts, 100)):
        for D, L, U in CELLS:
            route, t = cell(D, L, U, M, N, a.settle, a.reps)
            row = dict(layout=layout, D=D, L=L, U=U, M=M, N=N, route=route, on_ms=t["on"], off_ms=t["off"],
                       speedup=t["off"][0] / t["on"][0])
            rows.append(row)
            print("%-10s D=%2d L=%d U=%2d M=%5d N=%6d  %-15s on %8.3f ms [%8.3f, %8.3f]  off %8.3f ms [%8.3f, %8.3f]  x %.2f"
                  % (layout, D, L, U, M, N, route, *t["on"], *t["off"], row["speedup"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
