#!/usr/bin/env python3
"""Per-context coupling flows above 16 units with fewer than 32 samples per context: one launch per call each way
(NormFlow.wide_context_rows / wide_context_training, csrc/flow_ctx_wide.hip + csrc/flow_ctx_wide_bwd.hip) against the
route the same call takes with the switches off, in one process.

Cells: D in {4, 5, 8, 32, 64} x U in {20, 64} x N in {1, 8, 31} at S = 2, L = 2, with M = 2^16 / N contexts (M N = 2^16;
--rows changes the product).  Ops: `log_prob` (no_grad), `sample` (nf.sample with frozen statistics, no_grad) and `train`
(forward + backward of -log_prob.mean() on materialised parameter rows that require grad, z a constant).
Protocol: after a warm-up of each side, A (switches off: the parent's route, never the code under test) and B (switches
on) alternate for --rounds rounds; a round times, between two events, as many calls as fill --fill seconds.  The launch
counters verify per round that A ran no launch of the new kernels and B exactly one per call and direction and no other
flow kernel.
Reported per cell and op: the median time of each side, their ratio, the spread (max - min) / median over the rounds of
each side and the verdict of the gate: B is offered where A / B exceeds 1 + the sum of the two spreads.  For information,
column C of the `log_prob` rows: wideflow_ops.wide_flow_log_prob_raw (all 2 S images per workgroup, eight waves on at
most two tiles) on the same inputs where wide_flow_supported -- what the layer-at-a-time mapping buys -- as C / B.
A class that NormFlow leaves on the old route (one sample per context above 48 units) is still measured:
its B is the ops entry, plus the base density for `sample`, as the family's arm would run it; those rows carry a *.
The table goes to stdout and to --out (default profiles/ctxwidebench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, ctxwide_ops, ops, wideflow_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--rows", type=int, default=1 << 16, help="M * N of every cell")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctxwidebench.txt"))
args = ap.parse_args()
assert args.rounds >= 3

WIDTHS, UNITS, SAMPLES = [4, 5, 8, 32, 64], [20, 64], [1, 8, 31]
S, L = 2, 2
lib = _lib.lib
WANT = {"log_prob": (1, 0, 0), "sample": (0, 1, 0), "train": (1, 0, 1)}  # launches of the new kernels per call


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


def switch(nf, on):
    nf.wide_context_rows = nf.wide_context_training = on


def measure(nf, fn, want):
    """rounds of A / B -> (times A, times B)"""
    reps = {}
    for on in (False, True):
        switch(nf, on)
        fn()
        fn()
        torch.cuda.synchronize()
        reps[on] = max(1, int(args.fill / timed(fn, 2)) + 1)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            switch(nf, on)
            c0, d0 = ctxwide_ops.launch_counts(), diag()
            times[on].append(timed(fn, reps[on]))
            moved = tuple(a - b for a, b in zip(ctxwide_ops.launch_counts(), c0))
            if on:  # the new route: one launch per call and direction, no other flow kernel
                assert moved == tuple(reps[on] * w for w in want) and diag() == d0, (moved, reps[on])
            else:   # the parent's route: the new kernels never ran
                assert moved == (0, 0, 0)
    switch(nf, False)
    return times[False], times[True]


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


lines = ["ctxwidebench: %s, rounds %d, >= %.1f s per timed block; S = %d, L = %d, M N = %d; A = switches off (the parent's "
         "route), B = wide_context_rows + wide_context_training, C = wide_flow_log_prob_raw (information only)"
         % (torch.cuda.get_device_name(0), args.rounds, args.fill, S, L, args.rows),
         "%-8s %3s %3s %6s %3s %10s %10s %7s %9s %9s %8s  %s" % ("op", "D", "U", "M", "N", "A ms", "B ms", "A/B", "spread A",
                                                                "spread B", "C/B", "gate")]
print("\n".join(lines), flush=True)
for D in WIDTHS:
    for U in UNITS:
        torch.manual_seed(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        g = torch.Generator().manual_seed(D)
        for b in nf._bn_layers():
            b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
        P = nf.D_params
        for N in SAMPLES:
            M = max(2, args.rows // N)
            params = torch.empty(M, P, device="cuda").normal_(0.0, 0.05)
            pg = params.clone().requires_grad_()
            z = torch.randn(M, N, D, device="cuda")

            def log_prob():
                with torch.no_grad():
                    nf.log_prob(z, params)

            def sample():
                with torch.no_grad():
                    nf.sample(N, params, freeze_bn=True)

            def train():
                pg.grad = None
                (-nf.log_prob(z, pg).mean()).backward()

            def entry_log_prob():  # the arms of `context_rows_wide`, for a class the route leaves out
                if nf.wide_context_rows:
                    ctxwide_ops.ctx_wide_log_prob_raw(z, params, *nf._flow_args())
                else:
                    log_prob()

            def entry_sample():
                if nf.wide_context_rows:
                    omega = torch.randn((M, N, D), device="cuda", dtype=torch.float32)
                    _, sld = ctxwide_ops.ctx_wide_forward_raw(omega, params, *nf._flow_args())
                    ops.base_log_density_f64(omega) - sld
                else:
                    sample()

            switch(nf, True)
            with torch.no_grad():
                left_out = nf._route("log_prob", z, params).family != "context_rows_wide"
            switch(nf, False)
            for name, fn in (("log_prob", entry_log_prob if left_out else log_prob),
                             ("sample", entry_sample if left_out else sample), ("train", train)):
                if name == "train" and not ctxwide_ops.ctx_wide_train_supported(D, S, L, U, N):
                    continue
                ta, tb = measure(nf, fn, WANT[name])
                a, b = statistics.median(ta), statistics.median(tb)
                c = ""
                if name == "log_prob" and wideflow_ops.wide_flow_supported(D, S, L, U):
                    args_c = (z, params) + nf._flow_args()
                    wideflow_ops.wide_flow_log_prob_raw(*args_c)
                    torch.cuda.synchronize()
                    reps = max(1, int(args.fill / timed(lambda: wideflow_ops.wide_flow_log_prob_raw(*args_c), 2)) + 1)
                    tc = statistics.median([timed(lambda: wideflow_ops.wide_flow_log_prob_raw(*args_c), reps)
                                            for _ in range(args.rounds)])
                    c = "%.2f" % (tc / b)
                line = "%-8s %3d %3d %6d %3d %10.3f %10.3f %7.2f %8.1f%% %8.1f%% %8s  %s" % (
                    name + ("*" if left_out and name != "train" else ""), D, U, M, N, a * 1e3, b * 1e3, a / b, 100 * spread(ta), 100 * spread(tb), c,
                    "offered" if a / b > 1.0 + spread(ta) + spread(tb) else "NOT FASTER")
                print(line, flush=True)
                lines.append(line)
            del params, pg, z
            torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
