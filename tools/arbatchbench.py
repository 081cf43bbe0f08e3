"""Time fresh-statistics sampling of an autoregressive flow -- z, log_q = nf(N), what cde(x, N) and every iteration of
efn.train_efn run -- with NormFlow.ar_batch_forward on (one C call each way, include/tnf_arbatch.h) against the same
flow with the switch off in the same process (the per-bijector composition: MAF, bn_batch_forward, affine, one autograd
node each).

    python tools/arbatchbench.py --all [--txt profiles/r18_arbatchbench.txt]
    python tools/arbatchbench.py --mode sample|train --layout shared|lfi|efn|rows [--n 262144] [--contexts 2000]
                                 [--reps 15] [--settle 5] [--ignore-limit] [--out FILE.json]

--mode sample: the call under torch.no_grad() (family ar_batch_chain); --mode train: the call, a loss of z and log_q, and
its gradient w.r.t. the parameters, no optimiser (family ar_batch_train).  In train mode a third variant, `off+`, is the
switch-off composition with NormFlow.ar_sample_training on (the MAF's one-kernel sampling backward of tnf_arsample.h).
Cells: (D, L, U) in (4, 2, 20), (6, 2, 15), (16, 2, 32), (21, 2, 42), (32, 2, 16) with one parameter row and N = --n
samples (--layout shared) or --contexts parameter rows x 100 samples (--layout lfi); --layout efn is the EFN notebook's
size, 100 contexts x 100 samples at D = 4, L = 2, U = 15; --layout rows walks the batch size between the two, 100 contexts
x 25 .. 1600 samples at (4, 2, 15) and (16, 2, 32).  Protocol: the variants are warmed up until the clocks have
settled (--settle steps), then timed in alternation, one step each per round, with device events; the figure is the
median of --reps rounds with the smallest and largest round beside it.  --ignore-limit (sample mode): the `on` variant
takes the chain at any batch size, where NormFlow itself offers it up to M N D = 160,000 (the measurement behind that
limit).  One mode and layout per process; --all is the driver: every step of STEPS as a child process under its own time
limit, stopping at the first one that fails or runs out of time, the lines collected in --txt."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from arsamplebench import CELLS, alternate  # noqa: E402


def cell(D, L, U, M, N, train, settle, reps, ignore_limit=False):
    fns, route = {}, None
    omega = torch.randn(M, N, D, device="cuda", generator=torch.Generator(device="cuda").manual_seed(D))
    wz, wl = torch.randn_like(omega), torch.randn(M, N, device="cuda", dtype=torch.float64)
    variants = (("off", False, False), ("on", True, False)) + ((("off+", False, True),) if train else ())
    for name, switch, ast in variants:
        np.random.seed(D)
        nf = tnf.NormFlow(D, True, "AR", 1, L, U)
        nf.ar_batch_forward, nf.ar_sample_training = switch, ast
        if switch and ignore_limit and not train:  # the plain chain beyond the batch size NormFlow offers it at
            nf._ar_batch_family = lambda z, p, facts: "ar_batch_chain"
        p = torch.tensor(np.random.RandomState(D).normal(0, 0.2, (M, nf.D_params)), dtype=torch.float32,
                         device="cuda").requires_grad_(train)
        if switch:
            with torch.set_grad_enabled(train):
                route = nf._route("forward", omega, p, freeze_bn=False).family

        def step(nf=nf, p=p):
            with torch.set_grad_enabled(train):
                z, lq = nf._forward_from(omega, p, freeze_bn=False)
                if train:
                    torch.autograd.grad((z * wz).sum() + (lq * wl).sum(), p)

        fns[name] = step
    return route, alternate(fns, settle, reps)


# (mode, layout, time limit in seconds) of --all; the plain chain is measured beyond NormFlow's own limit too
STEPS = (("sample", "efn", 120), ("train", "efn", 120), ("sample", "rows", 150), ("sample", "shared", 150),
         ("sample", "lfi", 150), ("train", "shared", 200), ("train", "lfi", 200))


def run_all(a):
    """Every step in a process of its own (this one never touches the GPU); nothing is started after a failure."""
    lines = []
    for mode, layout, limit in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--layout", layout, "--n", str(a.n),
               "--contexts", str(a.contexts), "--reps", str(a.reps), "--settle", str(a.settle)]
        if mode == "sample":
            cmd.append("--ignore-limit")
        try:
            r = subprocess.run(cmd, timeout=limit, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            sys.exit("arbatchbench: %s %s ran past %d s; stopping" % (mode, layout, limit))
        print(r.stdout, end="", flush=True)
        if r.returncode:
            sys.exit("arbatchbench: %s %s ended with status %d; stopping" % (mode, layout, r.returncode))
        lines.append(r.stdout)
    if a.txt:
        with open(a.txt, "w") as f:
            f.write("".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--txt", default=None)
    ap.add_argument("--mode", choices=("sample", "train"))
    ap.add_argument("--layout", choices=("shared", "lfi", "efn", "rows"))
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--contexts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--settle", type=int, default=5)
    ap.add_argument("--ignore-limit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    if not (a.mode and a.layout):
        ap.error("--mode and --layout, or --all")
    train = a.mode == "train"
    cells = {"shared": [(c, 1, a.n) for c in CELLS], "lfi": [(c, a.contexts, 100) for c in CELLS],
             "efn": [((4, 2, 15), 100, 100)],
             "rows": [(c, 100, N) for c in ((4, 2, 15), (16, 2, 32)) for N in (25, 100, 400, 1600)]}[a.layout]
    rows = []
    for (D, L, U), M, N in cells:
        route, t = cell(D, L, U, M, N, train, a.settle, a.reps, a.ignore_limit)
        # adopt where the new route's slowest round beats the other's fastest
        row = dict(mode=a.mode, layout=a.layout, D=D, L=L, U=U, M=M, N=N, route=route, ms=t,
                   speedup=t["off"][0] / t["on"][0], clear_win=t["on"][2] < t["off"][1])
        rows.append(row)
        extra = "  off+ %8.3f ms [%8.3f, %8.3f]" % t["off+"] if "off+" in t else ""
        print("%-6s %-6s D=%2d L=%d U=%2d M=%5d N=%6d  %-14s on %8.3f ms [%8.3f, %8.3f]  off %8.3f ms [%8.3f, %8.3f]%s  x %.2f %s"
              % (a.mode, a.layout, D, L, U, M, N, route, *t["on"], *t["off"], extra, row["speedup"],
                 "clear" if row["clear_win"] else "NOT CLEAR"), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
