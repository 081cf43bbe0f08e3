"""Time a training step (log_prob forward and backward, no optimiser) of a coupling flow at the widths between the MFMA
shapes, with NormFlow.padded_training on -- padded whole-flow forward, the one-kernel reversible backward at the embedded
width 2H (include/tnf_padtrain.h) -- against the same flow with the switch off in the same process (the route these
widths take otherwise: one kernel per bijector each way, or the per-layer pair), at N = 2^19, S = 4, L = 2, U = 15.

    python tools/padded_train_bench.py [--n 524288] [--reps 20] [--d 4 8 16 31 48 63] [--skip-off] [--out FILE.json]

Protocol: every variant is warmed up until the clocks have settled (--settle steps), then the variants are timed in
alternation, one step each per round, with device events; the figure is the median of --reps rounds.  "on" is the
default overflow recovery ("device": the gated fp32 recomputation is enqueued behind every backward), "on/off-recovery"
the route without it.  The four layout kernels are timed alone as well, the row kernels against the 4 R (D + 2H) bytes
they move.  Prints one line per width and writes everything to --out as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib as L_  # noqa: E402
from torch_nf_amd import padtrain_ops as PT  # noqa: E402


INNER = 10  # launches per timed window of a kernel timed alone


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
    ap.add_argument("--d", type=int, nargs="*", default=[4, 8, 16, 31, 48, 63])
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-off", action="store_true",
                    help="time only the two on variants (no switch-off step between them: its buffers leave the "
                         "caching allocator in another state)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("padded_train_bench: needs a HIP device (a timing on the CPU says nothing)")
    S, L, U, N = 4, 2, 15, args.n
    torch.cuda.set_device(0)
    fn_cls = PT._FlowPaddedLogProbFn
    rows = []
    print("# N = %d, S = %d, L = %d, U = %d; median of %d alternating rounds after %d settling rounds; ms per step"
          % (N, S, L, U, args.reps, args.settle))
    print("%-3s %9s %9s %9s %8s %9s | %8s %8s %7s %7s %8s %8s" % (
        "D", "off", "on", "on/norec", "speedup", "grad_rel", "embed_us", "gather_us", "GB/s", "GB/s", "pemb_us", "pgat_us"))
    for D in args.d:
        rng = np.random.RandomState(D)
        nf = tnf.NormFlow(D, True, "coupling", S, L, U)
        P = L_.lib.tnf_flow_num_params(D, S, L, U)
        p = torch.from_numpy(rng.normal(0.0, 0.1, (1, P)).astype(np.float32)).cuda().requires_grad_()
        for b in nf._bn_layers():
            b.set_last_stats(torch.from_numpy(rng.normal(0.0, 0.3, D).astype(np.float32)).cuda(),
                             torch.from_numpy(np.exp(rng.normal(0.0, 0.2, D)).astype(np.float32)).cuda())
        z = torch.from_numpy(rng.normal(0.0, 1.0, (1, N, D)).astype(np.float32)).cuda()

        def step(switch, recovery="device"):
            nf.padded_training = switch
            fn_cls.overflow_recovery = recovery
            p.grad = None
            (-nf.log_prob(z, p).mean()).backward()
            fn_cls.overflow_recovery = "device"
            return p.grad

        nf.padded_training = True
        assert nf._train_path(z, p) == "padded", "D = %d is outside the feature" % D
        nf.padded_training = False
        route_off = nf._route("log_prob", z, p).family
        g_on, g_off = step(True).clone(), step(False).clone()
        grad_rel = float((g_on - g_off).abs().max() / g_off.abs().max())
        flag = int(fn_cls.last_overflow_flag.item())  # of the step(True) above: 0 = the one-kernel result stands
        variants = {"off": lambda: step(False), "on": lambda: step(True), "on_norec": lambda: step(True, "off")}
        if args.skip_off:
            del variants["off"]
        med, span = alternate(variants, args.settle, args.reps)
        med.setdefault("off", float("nan"))
        # the four kernels alone, on preallocated buffers, INNER launches per timed window
        W = PT.padded_width(D)
        rows_r = z.view(N, D)
        emb, back = PT.embed_rows_raw(rows_r, D), torch.empty_like(rows_r)
        mean, alpha = nf._bn_stats(torch.device("cuda", 0))
        pd = p.detach()
        pe, mean_e, alpha_e = PT.embed_params_raw(pd, P, mean, alpha, D, S, L, U)
        gp = torch.zeros_like(pd)
        lib, st = L_.lib, L_.stream_ptr()

        def many(call):
            def run():
                for _ in range(INNER):
                    L_.check(call())
            return run

        kmed, _ = alternate({
            "embed_rows": many(lambda: lib.tnf_flow_padded_embed_rows_f32(rows_r.data_ptr(), emb.data_ptr(), N, D, st)),
            "gather_rows": many(lambda: lib.tnf_flow_padded_gather_rows_f32(emb.data_ptr(), back.data_ptr(), N, D, st)),
            "embed_params": many(lambda: lib.tnf_flow_padded_embed_params_f32(
                pd.data_ptr(), mean.data_ptr(), alpha.data_ptr(), pe.data_ptr(), mean_e.data_ptr(), alpha_e.data_ptr(), 1, D, S,
                L, U, P, st)),
            "gather_params": many(lambda: lib.tnf_flow_padded_gather_params_f32(pe.data_ptr(), gp.data_ptr(), 1, D, S, L, U, P,
                                                                                  st))}, 2, args.reps)
        kmed = {k: v / INNER for k, v in kmed.items()}
        row_bytes = 4 * N * (D + W)
        r = dict(D=D, width=W, N=N, S=S, L=L, U=U, route_off=route_off,
                 step_ms=med, step_ms_min_max=span, speedup=med["off"] / med["on"],
                 speedup_without_recovery=med["off"] / med["on_norec"], grad_max_rel_on_vs_off=grad_rel, overflow_flag=flag,
                 kernel_us={k: 1e3 * v for k, v in kmed.items()}, row_bytes=row_bytes,
                 embed_rows_GBps=row_bytes / kmed["embed_rows"] / 1e6, gather_rows_GBps=row_bytes / kmed["gather_rows"] / 1e6,
                 note="kernel_us: %d back-to-back launches per timed window, launch gaps included" % INNER)
        rows.append(r)
        print("%-3d %9.3f %9.3f %9.3f %8.2f %9.2e | %8.1f %8.1f %7.0f %7.0f %8.1f %8.1f" % (
            D, med["off"], med["on"], med["on_norec"], r["speedup"], grad_rel, r["kernel_us"]["embed_rows"],
            r["kernel_us"]["gather_rows"], r["embed_rows_GBps"], r["gather_rows_GBps"], r["kernel_us"]["embed_params"],
            r["kernel_us"]["gather_params"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), reps=args.reps, settle=args.settle, rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
