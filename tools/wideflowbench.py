#!/usr/bin/env python3
"""Coupling flows with 17 <= num_units <= 64: the one-launch whole-flow wide kernel (NormFlow.wide_flow,
csrc/flow_wide.hip) against the route the same call takes with the switch off -- the wide per-layer chain at D % 8 == 0,
the per-bijector composition at every other D -- in one process.

Cells: (D, S, L, U) in {(4, 1, 2, 20) (the reference's own conditional-flow test), (5, 1, 2, 20), (8, 1, 2, 20),
(32, 4, 2, 32), (64, 2, 2, 32), (64, 1, 2, 64), (33, 2, 2, 20)}, each at (M, N) = (1, 2^17), (1, 2^20) and per-context rows
(2000, 100).  Operations: nf.log_prob(z, params) and nf._forward_from(omega, params, freeze_bn=True) (a float32 device
draw), under no_grad.  --cells picks cells by index, so that one invocation can be one GPU step with a time limit of its
own; the table is appended to --out.
Protocol: after a warm-up of each side, A (switch off) and B (switch on) alternate for --rounds rounds; a round times,
between two events, as many calls as fill --fill seconds.  The launch counters verify per round that A ran no launch of
the new kernel and B exactly one per call and no other flow kernel.  A row marked * is a class that `_wide_flow_ok` leaves
to today's route: B is then the ops entry plus the base density, as the `wide_flow` arm would run it, so that the class
stays measured.
Reported per row: the median time of each side, their ratio, the spread (max - min) / median over the rounds of each
side, and B as a fraction of its two bounds:
    byte bound   M N (8 D + 4) bytes / 8 TB/s: every sample read and written once, and its log-density;
    MFMA bound   M ceil(N / 16) tiles x 2 S layers x 16 (HT UT + (L - 1) UT UT / 2) v_mfma_f32_16x16x4_f32
                 (csrc/coupling_wide.hip) x 32 cycles per SIMD / (1024 SIMDs x 2.4 GHz).
The table goes to stdout and to --out (default profiles/wideflowbench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, wideflow_ops  # noqa: E402

SHAPES = [(4, 1, 2, 20), (5, 1, 2, 20), (8, 1, 2, 20), (32, 4, 2, 32), (64, 2, 2, 32), (64, 1, 2, 64), (33, 2, 2, 20)]
ROWS = [(1, 1 << 17), (1, 1 << 20), (2000, 100)]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--cells", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wideflowbench.txt"))
ap.add_argument("--small", action="store_true", help="N / 64 of every M = 1 row: a quick look, not a measurement")
args = ap.parse_args()
assert args.rounds >= 3

HBM, SIMDS, CLOCK, MFMA_CYCLES = 8.0e12, 1024, 2.4e9, 32
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
        nf.wide_flow = on
        fn()
        fn()
        torch.cuda.synchronize()
        reps[on] = max(1, int(args.fill / timed(fn, 2)) + 1)
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            nf.wide_flow = on
            c0, d0 = wideflow_ops.launch_counts(), diag()
            times[on].append(timed(fn, reps[on]))
            moved = wideflow_ops.launch_counts()[which] - c0[which]
            if on:  # the new route: one launch per call, no other flow kernel
                assert moved == reps[on] and diag() == d0, (moved, reps[on])
            else:   # the parent's route: the new kernel never ran
                assert moved == 0
    return times[False], times[True]


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def mfma_bound(M, N, D, S, L, U):
    HT, UT = ((D + 1) // 2 + 15) // 16, (U + 15) // 16
    per_layer = 2 * 4 * (HT * UT + (L - 1) * UT * UT + HT * UT)
    return M * ((N + 15) // 16) * 2 * S * per_layer * MFMA_CYCLES / (SIMDS * CLOCK)


cells = [int(i) for i in args.cells.split(",")]
lines = []
if cells[0] == 0:
    lines += ["wideflowbench: %s, rounds %d, >= %.1f s per timed block; A = switch off (the parent's route), B = wide_flow"
              % (torch.cuda.get_device_name(0), args.rounds, args.fill),
              "%2s %1s %1s %2s %5s %8s %-8s %10s %10s %7s %9s %9s %10s %10s" % (
                  "D", "S", "L", "U", "M", "N", "op", "A ms", "B ms", "A/B", "spread A", "spread B", "byte bound", "MFMA bound")]
print("\n".join(lines), flush=True)
with torch.no_grad():
    for D, S, L, U in (SHAPES[i] for i in cells):
        torch.manual_seed(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        g = torch.Generator().manual_seed(D)
        for b in nf._bn_layers():
            b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
        assert wideflow_ops.wide_flow_supported(D, S, L, U)
        for M, N in ROWS:
            if args.small and M == 1:
                N //= 64
            params = torch.empty(M, nf.D_params, device="cuda").normal_(0.0, 0.05)
            omega = torch.randn(M, N, D, device="cuda")
            nf.wide_flow = True
            z, _ = nf._forward_from(omega, params, freeze_bn=True)
            def sample_entry():  # what NormFlow's `wide_flow` arm does, for a class the route leaves out
                _, sld = wideflow_ops.wide_flow_forward_raw(omega, params, *nf._flow_args())
                return tnf.ops.base_log_density_f64(omega) - sld

            for op, which, fn in (("log_prob", 0, lambda: nf.log_prob(z, params)),
                                  ("sample", 1, lambda: nf._forward_from(omega, params, freeze_bn=True))):
                left_out = nf._route("forward" if which else "log_prob", omega, params, f32_draw=True).family != "wide_flow"
                if left_out:  # B = the entry itself, so that the class stays measured
                    assert which == 1
                    op, route_fn = op + "*", fn
                    fn = lambda: sample_entry() if nf.wide_flow else route_fn()  # noqa: E731
                ta, tb = measure(nf, fn, which)
                a, b = statistics.median(ta), statistics.median(tb)
                line = "%2d %1d %1d %2d %5d %8d %-8s %10.3f %10.3f %7.2f %8.1f%% %8.1f%% %9.1f%% %9.1f%%" % (
                    D, S, L, U, M, N, op, a * 1e3, b * 1e3, a / b, 100 * spread(ta), 100 * spread(tb),
                    100 * M * N * (8.0 * D + 4.0) / HBM / b, 100 * mfma_bound(M, N, D, S, L, U) / b)
                print(line, flush=True)
                lines.append(line)
            del params, omega, z
            torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if cells[0] else "w") as f:
    f.write("\n".join(lines) + "\n")
