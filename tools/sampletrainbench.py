"""Time a reparameterised step -- z, log_q = nf.sample(N) with frozen statistics under autograd, a loss of both, backward
(no optimiser) -- of a coupling flow with NormFlow.sample_training on (one sampling launch forward, the one walk kernel
of include/tnf_sampletrain.h backward) against the same flow with the switch off in the same process (the route such a
call takes otherwise: one kernel per bijector each way, every intermediate state kept), at S = 4, L = 2, U = 15.

    python tools/sampletrainbench.py [--n 524288] [--reps 20] [--d 4 16 31 32 48 63 64] [--no-rows] [--out FILE.json]

Cells: one shared parameter row with N = --n samples at every width of --d, and one per-row cell (D = 64, M = M_p = 64
parameter rows, N = 8192 samples each).  Protocol: every variant is warmed up until the clocks have settled (--settle
steps), then the variants are timed in alternation, one step each per round, with device events; the figure is the median
of --reps rounds, with the smallest and largest round beside it.  "on" is the default overflow recovery ("host": the flag
is read back after every backward), "on/no-recovery" the route without it.  The gate of DESIGN.md 20: in a cell the
route takes, the slowest "on" round is faster than the fastest "off" round.  Prints one line per cell and writes
everything to --out as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib as L_  # noqa: E402
from torch_nf_amd import sampletrain_ops as ST  # noqa: E402


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


def cell(D, S, L, U, M, N, settle, reps):
    rng = np.random.RandomState(D)
    P = L_.lib.tnf_flow_num_params(D, S, L, U)
    p = torch.tensor(rng.normal(0, 0.05, (M, P)), dtype=torch.float32, device="cuda").requires_grad_()
    omega = torch.randn(M, N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(D))
    stats = [(torch.tensor(rng.normal(0, 0.1, D)).float().cuda(), torch.tensor(rng.uniform(0.8, 1.25, D)).float().cuda())
             for _ in range(2 * S)]
    flows = {}
    for switch in (False, True):
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        for b, (m, al) in zip(nf._bn_layers(), stats):
            b.set_last_stats(m, al)
        nf.sample_training = switch
        flows[switch] = nf
    family = flows[True]._route("forward", omega, p, f32_draw=True).family

    def step(nf, mode):
        def run():
            ST._FlowSampleFn.overflow_recovery = mode
            p.grad = None
            z, log_q = nf._forward_from(omega, p, freeze_bn=True)  # nf.sample(N) with the draw held fixed
            (z.square().mean() + log_q.mean()).backward()
        return run

    fns = {"off": step(flows[False], "host"), "on": step(flows[True], "host"), "on/no-recovery": step(flows[True], "off")}
    before = ST.sample_train_launch_count()
    try:
        t = alternate(fns, settle, reps)
    finally:
        ST._FlowSampleFn.overflow_recovery = "host"
    calls = ST.sample_train_launch_count() - before
    g_on = p.grad.clone()
    fns["off"]()
    torch.cuda.synchronize()
    diff = float((g_on - p.grad).abs().max() / p.grad.abs().max())
    return dict(D=D, S=S, L=L, U=U, M=M, N=N, family=family, ms=t, walk_calls=calls, grad_diff_on_vs_off=diff,
                speedup=t["off"][0] / t["on"][0], gate=bool(t["on"][2] < t["off"][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle", type=int, default=10)
    ap.add_argument("--d", type=int, nargs="*", default=[4, 16, 31, 32, 48, 63, 64])
    ap.add_argument("--no-rows", action="store_true", help="leave the per-row cell (D = 64, M = 64, N = 8192) out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, L, U = 4, 2, 15
    cells = [(D, 1, a.n) for D in a.d] + ([] if a.no_rows else [(64, 64, 8192)])
    res = []
    print("%3s %3s %8s %-12s %26s %26s %26s %7s %5s %9s" % ("D", "M", "N", "family", "off ms (min..max)", "on ms (min..max)",
                                                         "on/no-recovery (min..max)", "off/on", "gate", "grad diff"))
    for D, M, N in cells:
        r = cell(D, S, L, U, M, N, a.settle, a.reps)
        res.append(r)
        f = lambda k: "%8.3f (%7.3f..%8.3f)" % r["ms"][k]  # noqa: E731
        print("%3d %3d %8d %-12s %26s %26s %26s %7.2f %5s %9.1e" % (D, M, N, r["family"], f("off"), f("on"),
                                                                  f("on/no-recovery"), r["speedup"],
                                                                  "held" if r["gate"] else "MISSED", r["grad_diff_on_vs_off"]),
              flush=True)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), S=S, L=L, U=U, reps=a.reps, settle=a.settle, cells=res), fh,
                      indent=1)


if __name__ == "__main__":
    main()
