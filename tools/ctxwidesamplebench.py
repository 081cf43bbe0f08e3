#!/usr/bin/env python3
"""Training per-context coupling flows above 16 units through their frozen-statistics samples, fewer than 32 draws per
context: one launch each way (NormFlow.wide_context_sample_training, csrc/flow_ctx_wide.hip forward +
csrc/flow_ctx_wide_sample_bwd.hip backward) against the route the same call takes with the switch off, in one process.

Cells: D in {4, 5, 8, 32, 64} x U in {20, 64} x N in {1, 8, 31} at S = 2, L = 2, with M = 2^16 / N contexts (M N = 2^16;
--rows changes the product).  The op is `train_sample`: z, log_q = nf._forward_from(omega, params, freeze_bn=True) on a
float32 device draw and materialised parameter rows that require grad, then ((z ** 2).sum() + log_q.sum()).backward().
Protocol: after a warm-up of each side, A (switch off: the parent's route, the per-bijector composition, never the code
under test) and B (switch on) alternate for --rounds rounds; a round times, between two events, as many calls as fill
--fill seconds.  The launch counters verify per round that A ran no launch of the new backward and B exactly one launch
of the wide sampling kernel and one of the new backward per call and no diag family.
Table 1, per cell: the median time of each side, their ratio, the spread (max - min) / median over the rounds of each
side, and the gate: B is offered where A / B exceeds 1 + the larger of the two spreads.
Table 2, per cell, from the same build: B under each forced team size (tnf_ctx_wide_sample_set_waves: 4, 8 and 16 waves,
alternating over the rounds), the automatic choice of the shipped rule (tnf_ctx_wide_sample_waves), the fastest team,
and the automatic choice's time over the fastest's.
Both tables go to stdout and to --out (default profiles/r23_ctxwidesamplebench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, ctxwide_ops, ctxwidesample_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--rows", type=int, default=1 << 16, help="M * N of every cell")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_ctxwidesamplebench.txt"))
args = ap.parse_args()
assert args.rounds >= 3

WIDTHS, UNITS, SAMPLES = [4, 5, 8, 32, 64], [20, 64], [1, 8, 31]
S, L = 2, 2
lib = _lib.lib


def diag():
    return [lib.tnf_diag_launch_count(f) for f in range(_lib.DIAG_FAMILIES)]


def new_counts():
    return ctxwide_ops.launch_counts()[ctxwide_ops.COUNT_FORWARD], ctxwidesample_ops.launch_count()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def fill_reps(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    return max(1, int(args.fill / timed(fn, 2)) + 1)


def measure(nf, fn):
    """rounds of A / B -> (times A, times B)"""
    reps = {}
    for on in (False, True):
        nf.wide_context_sample_training = on
        reps[on] = fill_reps(fn)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            nf.wide_context_sample_training = on
            c0, d0 = new_counts(), diag()
            times[on].append(timed(fn, reps[on]))
            moved = tuple(a - b for a, b in zip(new_counts(), c0))
            if on:  # the new route: one launch per call and direction, no other flow kernel
                assert moved == (reps[on], reps[on]) and diag() == d0, (moved, reps[on])
            else:   # the parent's route: the new kernels never ran
                assert moved == (0, 0), moved
    nf.wide_context_sample_training = False
    return times[False], times[True]


def measure_teams(nf, fn):
    """rounds of B under each forced team -> {waves: times}"""
    nf.wide_context_sample_training = True
    times = {w: [] for w in ctxwidesample_ops.TEAMS}
    try:
        reps = {}
        for w in ctxwidesample_ops.TEAMS:
            ctxwidesample_ops.set_waves(w)
            reps[w] = fill_reps(fn)
        for _ in range(args.rounds):
            for w in ctxwidesample_ops.TEAMS:
                ctxwidesample_ops.set_waves(w)
                c0 = new_counts()
                times[w].append(timed(fn, reps[w]))
                assert tuple(a - b for a, b in zip(new_counts(), c0)) == (reps[w], reps[w])
    finally:
        ctxwidesample_ops.set_waves(0)
        nf.wide_context_sample_training = False
    return times


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


head = ["ctxwidesamplebench: %s, rounds %d, >= %.1f s per timed block; S = %d, L = %d, M N = %d; op train_sample = forward + "
        "backward of sum z^2 + sum log_q; A = switch off (the parent's route), B = wide_context_sample_training"
        % (torch.cuda.get_device_name(0), args.rounds, args.fill, S, L, args.rows)]
t1 = ["table 1: A against B (automatic team)",
      "%3s %3s %6s %3s %10s %10s %7s %9s %9s %5s  %s" % ("D", "U", "M", "N", "A ms", "B ms", "A/B", "spread A", "spread B",
                                                       "team", "gate")]
t2 = ["table 2: B under each forced team size, the same build (ms, spread)",
      "%3s %3s %6s %3s %18s %18s %18s %5s %5s %9s" % ("D", "U", "M", "N", "4 waves", "8 waves", "16 waves", "auto", "best",
                                                     "auto/best")]


def flush():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + t1 + [""] + t2) + "\n")


print("\n".join(head), flush=True)
for D in WIDTHS:
    for U in UNITS:
        torch.manual_seed(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        g = torch.Generator().manual_seed(D)
        for b in nf._bn_layers():
            b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
        P = nf.D_params
        for N in SAMPLES:
            if not ctxwidesample_ops.ctx_wide_sample_supported(D, S, L, U, N):
                continue
            M = max(2, args.rows // N)
            pg = torch.empty(M, P, device="cuda").normal_(0.0, 0.05).requires_grad_()
            omega = torch.randn(M, N, D, device="cuda")

            def train_sample():
                pg.grad = None
                z, log_q = nf._forward_from(omega, pg, True)
                ((z ** 2).sum() + log_q.sum()).backward()

            ta, tb = measure(nf, train_sample)
            a, b = statistics.median(ta), statistics.median(tb)
            auto = ctxwidesample_ops.waves(D, U, N)
            line = "%3d %3d %6d %3d %10.3f %10.3f %7.2f %8.1f%% %8.1f%% %5d  %s" % (
                D, U, M, N, a * 1e3, b * 1e3, a / b, 100 * spread(ta), 100 * spread(tb), auto,
                "offered" if a / b > 1.0 + max(spread(ta), spread(tb)) else "NOT FASTER")
            print(line, flush=True)
            t1.append(line)
            tw = measure_teams(nf, train_sample)
            med = {w: statistics.median(ts) for w, ts in tw.items()}
            best = min(med, key=med.get)
            line = "%3d %3d %6d %3d %s %5d %5d %9.2f" % (
                D, U, M, N, " ".join("%10.3f %6.1f%%" % (med[w] * 1e3, 100 * spread(tw[w])) for w in ctxwidesample_ops.TEAMS),
                auto, best, med[auto] / med[best])
            print("  teams " + line, flush=True)
            t2.append(line)
            flush()
            del pg, omega
            torch.cuda.empty_cache()
flush()
