#!/usr/bin/env python3
"""Coupling flows with 17 <= num_units <= 64 at stage counts the resident whole-flow kernel cannot hold: the streamed
one-launch kernel (NormFlow.wide_flow_streamed, csrc/flow_wide_stream.hip) against the route the same call takes with
the switch off -- the wide per-layer chain at D % 8 == 0, the per-bijector composition at every other D -- in one
process.

Cells: (D, S, L, U) in {(64, 4, 2, 64) (the headline model at 64 units), (64, 4, 2, 32), (32, 8, 2, 32), (33, 4, 2, 20),
(5, 5, 2, 20), (64, 1, 3, 64)}, each at (M, N) = (1, 2^12), (1, 2^17), (1, 2^20) and per-context rows (2000, 100).  Operations:
nf.log_prob(z, params) and nf._forward_from(omega, params, freeze_bn=True) (a float32 device draw), under no_grad.
--cells picks cells by index, so that one invocation can be one GPU step with a time limit of its own; the table is
appended to --out.
Protocol: after a warm-up of each side, A (switch off) and B (switch on, at each shipped T forced through
tnf_wide_flow_stream_set_tiles; a T the tile shape does not have runs as its largest and is marked "=") alternate for
--rounds rounds; a round times, between two events, as many calls as fill --fill seconds.  The launch counters verify
per round that A ran no launch of the new kernel and B exactly one per call and no other flow kernel.  A row marked * is
a class that `_wide_flow_stream_ok` leaves to today's route: B is then the ops entry plus the base density, as the
`wide_flow_streamed` arm would run it, so that the class stays measured.
Reported per row: the median time of A and of B at each T, the T the rule picks and A / B at it, the largest spread
(max - min) / median over the rounds of A and of the B's, and B (at the rule's T) as a fraction of its MFMA bound,
    M ceil(N / 16) tiles x 2 S layers x 16 (HT UT + (L - 1) UT UT / 2) v_mfma_f32_16x16x4_f32 (csrc/coupling_wide.hip)
    x 32 cycles per SIMD / (1024 SIMDs x 2.4 GHz).
The table goes to stdout and to --out (default profiles/widestreambench.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, wideflow_ops, widestream_ops  # noqa: E402

SHAPES = [(64, 4, 2, 64), (64, 4, 2, 32), (32, 8, 2, 32), (33, 4, 2, 20), (5, 5, 2, 20), (64, 1, 3, 64)]
ROWS = [(1, 1 << 12), (1, 1 << 17), (1, 1 << 20), (2000, 100)]
TILES = widestream_ops.SHIPPED_TILES

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--fill", type=float, default=0.2)
ap.add_argument("--cells", default=",".join(str(i) for i in range(len(SHAPES))), help="indices into the shape list")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "widestreambench.txt"))
ap.add_argument("--small", action="store_true", help="N / 64 of every M = 1 row: a quick look, not a measurement")
args = ap.parse_args()
assert args.rounds >= 3

SIMDS, CLOCK, MFMA_CYCLES = 1024, 2.4e9, 32
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


def side(nf, key):
    """key: 0 = A (switch off), T = B with T tiles per wave forced."""
    nf.wide_flow_streamed = key != 0
    widestream_ops.set_tiles(key)


def measure(nf, fn, which):
    """rounds of A / B(T) ... -> {key: times}"""
    keys = (0,) + TILES
    reps = {}
    for k in keys:
        side(nf, k)
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(1, int(args.fill / timed(fn, 2)) + 1)
    times = {k: [] for k in keys}
    for _ in range(args.rounds):
        for k in keys:
            side(nf, k)
            c0, d0, w0 = widestream_ops.launch_counts(), diag(), wideflow_ops.launch_counts()
            times[k].append(timed(fn, reps[k]))
            moved = widestream_ops.launch_counts()[which] - c0[which]
            if k:  # the new route: one launch per call, no other flow kernel
                assert moved == reps[k] and diag() == d0 and wideflow_ops.launch_counts() == w0, (moved, reps[k])
            else:  # the parent's route: the new kernel never ran
                assert moved == 0
    side(nf, 0)
    return times


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


def mfma_bound(M, N, D, S, L, U):
    HT, UT = ((D + 1) // 2 + 15) // 16, (U + 15) // 16
    per_layer = 2 * 4 * (HT * UT + (L - 1) * UT * UT + HT * UT)
    return M * ((N + 15) // 16) * 2 * S * per_layer * MFMA_CYCLES / (SIMDS * CLOCK)


def max_tiles(D, L, U):  # wide_stream_max_tiles (csrc/wide_stream.h)
    HT, UT = ((D + 1) // 2 + 15) // 16, (U + 15) // 16
    return (1 if L > 3 else 2) if (HT, UT) == (2, 4) else 4


cells = [int(i) for i in args.cells.split(",")]
lines = []
if cells[0] == 0:
    lines += ["widestreambench: %s, rounds %d, >= %.1f s per timed block; A = switch off (the parent's route), "
              "B = wide_flow_streamed at T tiles per wave" % (torch.cuda.get_device_name(0), args.rounds, args.fill),
              "%2s %1s %1s %2s %5s %8s %-8s %10s " % ("D", "S", "L", "U", "M", "N", "op", "A ms")
              + " ".join("%10s" % ("B(T=%d) ms" % t) for t in TILES)
              + " %4s %7s %9s %9s %10s" % ("rule", "A/B", "spread A", "spread B", "MFMA bound")]
print("\n".join(lines), flush=True)
with torch.no_grad():
    for D, S, L, U in (SHAPES[i] for i in cells):
        torch.manual_seed(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        g = torch.Generator().manual_seed(D)
        for b in nf._bn_layers():
            b.set_last_stats((torch.randn(D, generator=g) * 0.1).cuda(), (torch.rand(D, generator=g) * 0.5 + 0.75).cuda())
        assert widestream_ops.wide_flow_stream_supported(D, S, L, U) and not wideflow_ops.wide_flow_supported(D, S, L, U)
        for M, N in ROWS:
            if args.small and M == 1:
                N //= 64
            params = torch.empty(M, nf.D_params, device="cuda").normal_(0.0, 0.05 * S ** -0.5)
            omega = torch.randn(M, N, D, device="cuda")
            z, _ = nf._forward_from(omega, params, freeze_bn=True)

            def sample_entry():  # what NormFlow's `wide_flow_streamed` arm does, for a class the route leaves out
                _, sld = widestream_ops.wide_flow_stream_forward_raw(omega, params, *nf._flow_args())
                return tnf.ops.base_log_density_f64(omega) - sld

            def log_prob_entry():
                return widestream_ops.wide_flow_stream_log_prob_raw(z, params, *nf._flow_args())[0]

            for op, which, fn, entry in (("log_prob", 0, lambda: nf.log_prob(z, params), log_prob_entry),
                                         ("sample", 1, lambda: nf._forward_from(omega, params, freeze_bn=True), sample_entry)):
                nf.wide_flow_streamed = True
                left_out = nf._route("forward" if which else "log_prob", omega, params, f32_draw=True).family != "wide_flow_streamed"
                if left_out:  # B = the entry itself, so that the class stays measured
                    op, route_fn = op + "*", fn
                    fn = lambda: entry() if nf.wide_flow_streamed else route_fn()  # noqa: E731
                t = measure(nf, fn, which)
                med = {k: statistics.median(v) for k, v in t.items()}
                rule, cap = widestream_ops.tiles(D, S, L, U, M, N), max_tiles(D, L, U)
                line = "%2d %1d %1d %2d %5d %8d %-8s %10.3f " % (D, S, L, U, M, N, op, med[0] * 1e3) + " ".join(
                    "%9.3f%s" % (med[k] * 1e3, "=" if k > cap else " ") for k in TILES) + " %4d %7.2f %8.1f%% %8.1f%% %9.1f%%" % (
                    rule, med[0] / med[rule], 100 * spread(t[0]), 100 * max(spread(t[k]) for k in TILES),
                    100 * mfma_bound(M, N, D, S, L, U) / med[rule])
                print(line, flush=True)
                lines.append(line)
            del params, omega, z
            torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if cells[0] else "w") as f:
    f.write("\n".join(lines) + "\n")
