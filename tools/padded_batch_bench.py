"""Time sampling with fresh batch statistics -- nf(N) with freeze_bn=False, alone (no autograd) and as a training step's
forward + backward -- of a coupling flow at the widths between the MFMA shapes, with NormFlow.padded_batch_forward on (the
batch-statistics chains at the embedded width 2H, include/tnf_padbatch.h) against the switch off in the same process (the
route these widths take otherwise: one kernel per bijector), at N = 2^19, S = 4, L = 2, U = 15.

    python tools/padded_batch_bench.py [--n 524288] [--reps 20] [--d 4 16 31 48 63] [--root DIR] [--out FILE.json]

--root DIR imports torch_nf_amd from another tree, e.g. a build of the parent commit: a package without the switch ignores
it, so only its "off" figures mean anything and only those are printed.

Protocol: every variant is warmed up until the clocks have settled (--settle rounds), then the variants are timed in
alternation, one call each per round, with device events; the figure is the median of --reps rounds.  The base draw is a
float32 device tensor (NormFlow.sample's), so no host draw and no copy is in the figures.  The loss of the training step is
mean(log_q) + mean(z^2).  Prints one line per width and writes everything to --out as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, settle, reps):
    """{name: median ms} of the callables, timed in alternation after `settle` untimed rounds."""
    for _ in range(settle):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}, {k: [float(min(v)), float(max(v))] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 19)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle", type=int, default=10)
    ap.add_argument("--d", type=int, nargs="*", default=[4, 16, 31, 48, 63])
    ap.add_argument("--root", default=HERE, help="the tree to import torch_nf_amd from (default: this one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch_nf_amd as tnf

    if not torch.cuda.is_available():
        sys.exit("padded_batch_bench: needs a HIP device (a timing on the CPU says nothing)")
    has_switch = hasattr(tnf.NormFlow, "_padded_batch_ok")
    S, L, U, N = 4, 2, 15, args.n
    torch.cuda.set_device(0)
    rows = []
    print("# package: %s%s" % (os.path.dirname(tnf.__file__), "" if has_switch else " (no switch: the off route only)"))
    print("# N = %d, S = %d, L = %d, U = %d; median of %d alternating rounds after %d settling rounds; ms per call"
          % (N, S, L, U, args.reps, args.settle))
    print("%-3s %10s %10s %8s %12s %12s %8s %10s %10s" % ("D", "fwd off", "fwd on", "speedup", "fwd+bwd off", "fwd+bwd on",
                                                        "speedup", "z_maxabs", "grad_rel"))
    for D in args.d:
        rng = np.random.RandomState(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        P = tnf._lib.lib.tnf_flow_num_params(D, S, L, U)
        p = torch.from_numpy(rng.normal(0.0, 0.1, (1, P)).astype(np.float32)).cuda().requires_grad_()
        omega = torch.from_numpy(rng.normal(0.0, 1.0, (1, N, D)).astype(np.float32)).cuda()

        def forward(switch):
            nf.padded_batch_forward = switch
            with torch.no_grad():
                return nf._forward_from(omega, p, freeze_bn=False)

        def step(switch):
            nf.padded_batch_forward = switch
            p.grad = None
            z, lq = nf._forward_from(omega, p, freeze_bn=False)
            (lq.mean() + (z ** 2).mean()).backward()
            return p.grad

        routes = {}
        for switch in ((False, True) if has_switch else (False,)):
            nf.padded_batch_forward = switch
            with torch.no_grad():
                routes["fwd_" + ("on" if switch else "off")] = nf._route("forward", omega, p, freeze_bn=False).family
            routes["step_" + ("on" if switch else "off")] = nf._route("forward", omega, p, freeze_bn=False).family
        z_err = grad_rel = float("nan")
        if has_switch:
            assert routes["fwd_on"] == "batch_chain_padded" and routes["step_on"] == "batch_train_padded", (D, routes)
            z_err = float((forward(True)[0] - forward(False)[0]).abs().max())
            g_on, g_off = step(True).clone(), step(False).clone()
            grad_rel = float((g_on - g_off).abs().max() / g_off.abs().max())
        variants = {"fwd_off": lambda: forward(False), "step_off": lambda: step(False)}
        if has_switch:
            variants.update({"fwd_on": lambda: forward(True), "step_on": lambda: step(True)})
        med, span = alternate(variants, args.settle, args.reps)
        for k in ("fwd_on", "step_on"):
            med.setdefault(k, float("nan"))
        r = dict(D=D, N=N, S=S, L=L, U=U, routes=routes, ms=med, ms_min_max=span, speedup_fwd=med["fwd_off"] / med["fwd_on"],
                 speedup_step=med["step_off"] / med["step_on"], z_max_abs_on_vs_off=z_err, grad_max_rel_on_vs_off=grad_rel)
        rows.append(r)
        print("%-3d %10.3f %10.3f %8.2f %12.3f %12.3f %8.2f %10.2e %10.2e" % (
            D, med["fwd_off"], med["fwd_on"], r["speedup_fwd"], med["step_off"], med["step_on"], r["speedup_step"], z_err,
            grad_rel), flush=True)
        del nf, p, omega
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), package=os.path.dirname(tnf.__file__), reps=args.reps,
                           settle=args.settle, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
