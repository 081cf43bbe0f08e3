"""Time the padded whole-flow kernel (tnf_flow_padded_*, NormFlow with fusion AUTO) against the path each shape took
before (fusion = FUSE_LAYER: the wide per-layer chain at D % 8 == 0, the per-bijector composition otherwise) and against
the exact D = 32 / 64 whole-flow kernels, at N = 2^20, S = 4, L = 2, U = 15: log_prob and frozen-statistics sampling
(the forward pass from a fixed float32 device draw).  Also checks that both paths agree on the same seeded inputs.

    python tools/padded_flow_bench.py [--n 1048576] [--reps 20] [--d 4 8 16 31 32 48 63 64]

One line per (D, op): M samples/s of each path, the speed-up, and the largest disagreement."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib as L_  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def rel(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp_min(1.0)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--d", type=int, nargs="*", default=[4, 8, 16, 31, 32, 48, 63, 64])
    args = ap.parse_args()
    S, L, U, N = 4, 2, 15, args.n
    torch.cuda.set_device(0)
    print("# N = %d, S = %d, L = %d, U = %d; median of %d; M samples/s" % (N, S, L, U, args.reps))
    print("%-4s %-9s %-10s %10s %10s %8s %10s" % ("D", "op", "path", "new", "replaced", "speedup", "max_rel"))
    for D in args.d:
        rng = np.random.RandomState(D)
        nf = tnf.NormFlow(D, False, "coupling", S, L, U)
        P = L_.lib.tnf_flow_num_params(D, S, L, U)
        nf.params = torch.from_numpy(rng.normal(0.0, 0.1, (1, P)).astype(np.float32)).cuda()
        for b in nf._bn_layers():
            b.set_last_stats(torch.from_numpy(rng.normal(0.0, 0.3, D).astype(np.float32)).cuda(),
                             torch.from_numpy(np.exp(rng.normal(0.0, 0.2, D)).astype(np.float32)).cuda())
        z = torch.from_numpy(rng.normal(0.0, 1.0, (1, N, D)).astype(np.float32)).cuda()
        exact = D in (32, 64)
        path = "exact" if exact else "padded"
        with torch.no_grad():
            for op in ("log_prob", "sample"):
                if op == "log_prob":
                    fn = lambda: nf.log_prob(z)  # noqa: E731
                else:
                    fn = lambda: nf._forward_from(z, nf.params, freeze_bn=True)  # noqa: E731
                nf.fusion = L_.FUSE_AUTO
                t_new = timed(fn, args.reps)
                out_new = fn()
                nf.fusion = L_.FUSE_LAYER
                t_old = timed(fn, args.reps)
                out_old = fn()
                nf.fusion = L_.FUSE_AUTO
                if op == "log_prob":
                    err = rel(out_new, out_old)
                else:
                    err = max(rel(out_new[0], out_old[0]), rel(out_new[1], out_old[1]))
                print("%-4d %-9s %-10s %10.0f %10.0f %8.2f %10.2e" % (
                    D, op, path, N / t_new / 1e3, N / t_old / 1e3, t_old / t_new, err), flush=True)


if __name__ == "__main__":
    main()
