"""Time the rejection-ABC kernel (one GPU process; every step under its own time limit, as in tools/mogbench.py):

  script  ABC_SMC at the shape of the reference's scripts/smcabc_mat.py: d = 2, T = 50, N = 50, sigma = 0.25, its
          tolerance schedule in this package's (det, trace) order; kernel time, trials/s, time per finished chain --
          and the wall time of the float64 restatement (tests/abc_restatement.py) on ONE CPU thread, 2^15 trials per
          round and chain (it evaluates whole blocks, so its figure is a rate per trial)
  wide    N = 2^16 chains from starting points that satisfy the tolerance, d in {2, 3, 6}, T = 16 rounds at one tolerance

    python tools/abcbench.py [--steps 5] [--limit 120] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")  # the CPU figure is a one-thread figure
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import abc_restatement as R  # noqa: E402
from mogbench import Watchdog  # noqa: E402
from torch_nf_amd import abc_ops  # noqa: E402
from torch_nf_amd.systems import Mat  # noqa: E402


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def timed_launch(fn, steps):
    fn()  # warm-up: code object load
    torch.cuda.synchronize()
    times = []
    for s in range(steps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn(s)
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) * 1e-3)
    return float(np.median(times)), out


def executed_trials(trials, max_trials):
    """Trials the kernel evaluated up to each acceptance, plus max_trials for the round in which a chain gave up."""
    dead = trials == 0
    gave_up = dead & ~np.concatenate((np.zeros((1, trials.shape[1]), dtype=bool), dead[:-1]))
    return int(trials.sum()) + int(gave_up.sum()) * max_trials


def start_points(d, N, x0, eps0, rng):
    out, n = [], 0
    while n < N:
        z = rng.uniform(-2.0, 2.0, (1 << 16, d * (d + 1) // 2))
        keep = z[np.all(np.abs(R.stats(z, d) - x0) < eps0, axis=-1)]
        out.append(keep)
        n += len(keep)
    return np.concatenate(out)[:N]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(1)
    # ---- the script's shape
    d, T, N, sigma, mt = 2, 50, 50, 0.25, 1 << 20
    mat = Mat(d)
    x0 = np.array([0.0, d / 2])
    eps = np.stack([np.linspace(e1, eT, T) for e1, eT in ((d / 2, 2.0), (2.0, 0.02))], axis=1)
    np.random.seed(1)
    z0 = mat.prior.rvs(N)
    args = (f32(z0), f32(sigma * np.eye(mat.D)), f32(np.stack((mat.lb, mat.ub))), f32(x0), f32(eps), d, mt)
    out = dict(case="script", d=d, T=T, N=N, sigma=sigma, max_trials=mt)
    with Watchdog(a.limit, out):
        t, (zs, xs, trials) = timed_launch(lambda s=0: abc_ops.abc_smc_mat(*args, seed=1000 + s), a.steps)
        trials = trials.cpu().numpy().astype(np.int64)
        n_trials = executed_trials(trials, mt)
        alive = int((trials[-1] > 0).sum())
        out.update(seconds=t, chains_that_gave_up=N - alive, trials=n_trials, trials_per_s=n_trials / t,
                   seconds_per_sample=t / max(1, alive),
                   last_round_acceptance=float(alive / max(1, trials[-1].sum())),
                   longest_finished_chain_trials=int(trials.sum(0).max()))
    print(json.dumps(out), flush=True)
    if not a.no_cpu:
        cpu = dict(case="script, float64 restatement, one CPU thread", seed=1000 + a.steps - 1)
        with Watchdog(2 * a.limit, cpu):
            # the restatement evaluates a whole block of trials per round and chain, accepted or not: its rate per trial
            block = 1 << 15
            t0 = time.perf_counter()
            R.smc_chain(z0.astype(np.float32), sigma * np.eye(mat.D), mat.lb, mat.ub, x0, eps, d, block, seed=cpu["seed"])
            tc = time.perf_counter() - t0
            cpu.update(seconds=tc, trials_per_round_and_chain=block, trials_evaluated=T * N * block,
                       trials_per_s=T * N * block / tc, kernel_trials_per_s_over_this=out["trials_per_s"] * tc / (T * N * block),
                       seconds_for_the_kernels_trials=n_trials * tc / (T * N * block))
        print(json.dumps(cpu), flush=True)
    # ---- wide
    rng = np.random.RandomState(0)
    for d, e in ((2, (1.0, 0.5)), (3, (1.5, 0.75)), (6, (20.0, 3.0))):
        N, T, mt = 1 << 16, 16, 1 << 16
        mat = Mat(d)
        x0 = np.array([0.0, d / 2])
        eps = np.tile(np.array(e), (T, 1))
        z0 = start_points(d, N, x0, eps[0], rng)
        args = (f32(z0), f32(0.5 * np.eye(mat.D)), f32(np.stack((mat.lb, mat.ub))), f32(x0), f32(eps), d, mt)
        out = dict(case="wide", d=d, D=mat.D, T=T, N=N, sigma=0.5, eps=list(e), max_trials=mt)
        with Watchdog(a.limit, out):
            t, (zs, xs, trials) = timed_launch(lambda s=0: abc_ops.abc_smc_mat(*args, seed=1000 + s), a.steps)
            trials = trials.cpu().numpy().astype(np.int64)
            n_trials = executed_trials(trials, mt)
            # a wave evaluates whole sweeps of 64 trials: the trials it computes, not only those up to the accepted one
            swept = int(((trials + 63) // 64 * 64).sum())
            out.update(seconds=t, chains_that_gave_up=int((trials[-1] == 0).sum()), trials=n_trials, trials_per_s=n_trials / t,
                       evaluated_trials=swept, evaluated_trials_per_s=swept / t, seconds_per_sample=t / (N * T),
                       acceptance=float(N * T / max(1, n_trials)))
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
