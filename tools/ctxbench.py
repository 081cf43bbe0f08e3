#!/usr/bin/env python3
"""Per-context coupling flows with fewer than 32 samples per context: the one-launch route (NormFlow.context_rows,
csrc/flow_ctx.hip) against the route the same call takes with the switch off, in one process.

Shapes: D = 64, S = 4, L = 2, U = 15 at (M, N) in {(2^17, 8), (2^20, 1), (2^16, 16), (2^15, 31)}; D = 4, S = 1 (the
LFI_gauss flow) and D = 6, S = 2 at (2^20, 1) and (2^17, 8); then the cells around the break-even with the fp32-MFMA layer
kernel of the old route: D = 64 at (2^19, 2), (2^18, 4), (2^18, 6) and D = 32 at (2^20, 1), (2^17, 8).  Operations: nf.log_prob(z, params) and
nf._forward_from(omega, params, freeze_bn=True) (a float32 device draw) on materialised parameter rows, under no_grad.
Protocol: after a warm-up of each side, A (switch off) and B (switch on) alternate for --rounds rounds; a round times,
between two events, as many calls as fill --fill seconds.  The launch counters verify per round that A ran no launch of
the new kernel and B exactly one per call and no other flow kernel.
Reported per row: the median time of each side, their ratio, the spread (max - min) / median over the rounds of each
side, M samples/s of the new route, and the achieved fraction of the BYTE BOUND
    M * 4 * (D_params + (N D + N  for log_prob | 2 N D  for sampling)) bytes / 8 TB/s
-- the time to move each parameter row and each sample once at the HBM peak, as a fraction of the measured time.
The table goes to stdout and to --out (default profiles/ctxbench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, ctxflow_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctxbench.txt"))
ap.add_argument("--small", action="store_true", help="M / 64 of every shape: a quick look, not a measurement")
args = ap.parse_args()
assert args.rounds >= 3

HBM = 8.0e12
SHAPES = [(64, 4, 1 << 17, 8), (64, 4, 1 << 20, 1), (64, 4, 1 << 16, 16), (64, 4, 1 << 15, 31),
          (4, 1, 1 << 20, 1), (4, 1, 1 << 17, 8), (6, 2, 1 << 20, 1), (6, 2, 1 << 17, 8),
          # where the old route is the fp32-MFMA layer kernel with one context per wave: the cells around its break-even
          (64, 4, 1 << 19, 2), (64, 4, 1 << 18, 4), (64, 4, 1 << 18, 6), (32, 4, 1 << 20, 1), (32, 4, 1 << 17, 8)]
L, U = 2, 15
lib = _lib.lib


def diag():
    return [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def measure(nf, fn, which):
    """rounds of A / B -> (times A, times B)"""
    reps = {}
    for on in (False, True):
        nf.context_rows = on
        fn()
        fn()
        torch.cuda.synchronize()
        reps[on] = max(1, int(args.fill / timed(fn, 2)) + 1)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            nf.context_rows = on
            c0, d0 = ctxflow_ops.launch_counts(), diag()
            times[on].append(timed(fn, reps[on]))
            moved = ctxflow_ops.launch_counts()[which] - c0[which]
            if on:  # the new route: one launch per call, no other flow kernel
                assert moved == reps[on] and diag() == d0, (moved, reps[on])
            else:   # the parent's route: the new kernel never ran
                assert moved == 0
    return times[False], times[True]


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


lines = ["ctxbench: %s, rounds %d, >= %.1f s per timed block; A = switch off (the parent's route), B = context_rows"
         % (torch.cuda.get_device_name(0), args.rounds, args.fill),
         "%3s %2s %8s %3s %-8s %10s %10s %7s %9s %9s %11s %10s" % ("D", "S", "M", "N", "op", "A ms", "B ms", "A/B", "spread A",
                                                                   "spread B", "B Msmp/s", "byte bound")]
print("\n".join(lines), flush=True)
gate = None
with torch.no_grad():
    for D, S, M, N in SHAPES:
        if args.small:
            M //= 64
        torch.manual_seed(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        g = torch.Generator().manual_seed(D)
        for b in nf._bn_layers():
            b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
        P = nf.D_params
        params = torch.empty(M, P, device="cuda").normal_(0.0, 0.05)
        omega = torch.randn(M, N, D, device="cuda")
        nf.context_rows = True
        z, _ = nf._forward_from(omega, params, freeze_bn=True)
        for op, which, fn, io in (("log_prob", 0, lambda: nf.log_prob(z, params), N * D + N),
                                  ("sample", 1, lambda: nf._forward_from(omega, params, freeze_bn=True), 2 * N * D)):
            ta, tb = measure(nf, fn, which)
            a, b = statistics.median(ta), statistics.median(tb)
            bound = M * 4.0 * (P + io) / HBM
            line = "%3d %2d %8d %3d %-8s %10.3f %10.3f %7.2f %8.1f%% %8.1f%% %11.1f %9.1f%%" % (
                D, S, M, N, op, a * 1e3, b * 1e3, a / b, 100 * spread(ta), 100 * spread(tb), M * N / b / 1e6, 100 * bound / b)
            print(line, flush=True)
            lines.append(line)
            if (D, M, N, op) == (64, 1 << 17, 8, "log_prob"):
                gate = (a, b, max(spread(ta), spread(tb)))
        del params, omega, z
        torch.cuda.empty_cache()
if gate is not None:
    a, b, sp = gate
    verdict = "holds" if a / b > 1.0 + sp else "FAILS"
    line = ("gate (D = 64, M = 2^17, N = 8, log_prob): B is %.2f x faster than A, the larger spread is %.1f %% -> %s; "
            "%.0f M samples/s (aim: 400)" % (a / b, 100 * sp, verdict, (1 << 17) * 8 / b / 1e6))
    print(line)
    lines.append(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
