#!/usr/bin/env python3
"""Training per-context coupling flows through their frozen-statistics samples with fewer than 32 draws per context: one
launch each way (NormFlow.context_sample_training, csrc/flow_ctx.hip + csrc/flow_ctx_sample_bwd.hip) against the route
the same step takes with the switch off, in one process.

Cells: D in {4, 6, 32, 64} x N in {1, 4, 8, 16, 31} at S = 4, L = 2, U = 15, with M = 2^16 / N contexts (M N = 2^16;
--rows changes the product).  A step is z, log_q = nf._forward_from(omega, params, freeze_bn=True) on a float32 device
draw and materialised parameter rows that require grad, then (mean z^2 + mean log_q).backward().
Protocol: after a warm-up of each side, A (switch off: the parent's route) and B (switch on) alternate for --rounds
rounds; a round times, between two events, as many steps as fill --fill seconds.  The launch counters verify per round
that A ran no launch of the per-context kernels and B exactly one forward and one backward launch per step and no other
flow kernel.
Reported per cell: the median time of each side, their ratio, the spread (max - min) / median over the rounds of each
side, M samples/s of the new route, the achieved fraction of the BYTE BOUND
    M * 4 * (3 D_params + 4 N D + 2 N) bytes / 8 TB/s
-- each parameter row read by both kernels and its gradient row written once, the draw read, z written and read, its
gradient read -- and the verdict of the gate: B is offered where A / B exceeds 1 + the larger spread.
The table goes to stdout and to --out (default profiles/ctxsamplebench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, ctxflow_ops, ctxsample_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--rows", type=int, default=1 << 16, help="M * N of every cell")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctxsamplebench.txt"))
args = ap.parse_args()
assert args.rounds >= 3

HBM = 8.0e12
WIDTHS = [4, 6, 32, 64]
SAMPLES = [1, 4, 8, 16, 31]
S, L, U = 4, 2, 15
lib = _lib.lib


def diag():
    return [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]


def counters():
    return ctxflow_ops.launch_counts()[1], ctxsample_ops.launch_count()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def measure(nf, fn):
    """rounds of A / B -> (times A, times B)"""
    reps = {}
    for on in (False, True):
        nf.context_sample_training = on
        fn()
        fn()
        torch.cuda.synchronize()
        reps[on] = max(1, int(args.fill / timed(fn, 2)) + 1)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            nf.context_sample_training = on
            c0, d0 = counters(), diag()
            times[on].append(timed(fn, reps[on]))
            moved = [a - b for a, b in zip(counters(), c0)]
            if on:  # the new route: one launch each way per step, no other flow kernel
                assert moved == [reps[on], reps[on]] and diag() == d0, (moved, reps[on])
            else:   # the parent's route: the per-context kernels never ran
                assert moved == [0, 0]
    return times[False], times[True]


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


lines = ["ctxsamplebench: %s, rounds %d, >= %.1f s per timed block; step = frozen-statistics sampling + backward of "
         "mean z^2 + mean log_q; A = switch off (the parent's route), B = context_sample_training"
         % (torch.cuda.get_device_name(0), args.rounds, args.fill),
         "%3s %2s %8s %3s %10s %10s %7s %9s %9s %11s %10s  %s" % ("D", "S", "M", "N", "A ms", "B ms", "A/B", "spread A", "spread B",
                                                                 "B Msmp/s", "byte bound", "gate")]
print("\n".join(lines), flush=True)
for D in WIDTHS:
    torch.manual_seed(D)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    g = torch.Generator().manual_seed(D)
    for b in nf._bn_layers():
        b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
    P = nf.D_params
    for N in SAMPLES:
        M = max(2, args.rows // N)
        params = torch.empty(M, P, device="cuda").normal_(0.0, 0.05).requires_grad_()
        omega = torch.randn(M, N, D, device="cuda")

        def step():
            params.grad = None
            z, log_q = nf._forward_from(omega, params, freeze_bn=True)
            (z.square().mean() + log_q.mean()).backward()

        ta, tb = measure(nf, step)
        a, b = statistics.median(ta), statistics.median(tb)
        sp = max(spread(ta), spread(tb))
        bound = M * 4.0 * (3 * P + 4 * N * D + 2 * N) / HBM
        line = "%3d %2d %8d %3d %10.3f %10.3f %7.2f %8.1f%% %8.1f%% %11.1f %9.1f%%  %s" % (
            D, S, M, N, a * 1e3, b * 1e3, a / b, 100 * spread(ta), 100 * spread(tb), M * N / b / 1e6, 100 * bound / b,
            "offered" if a / b > 1.0 + sp else "NOT FASTER")
        print(line, flush=True)
        lines.append(line)
        del params, omega
        torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
