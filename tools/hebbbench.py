"""Time the Hebbian learning-rule simulator and the train_nde step around it (one GPU process; every measurement under
its own time limit, as in tools/mogbench.py).  Each figure is the median of --reps timed windows after warm-up, with the
spread (min .. max) beside it; the clock is settled by the warm-up windows (tools/clock_ramp.py: some 0.2 s of work).

  kernel  tnf_hebb_simulate_f32 at (N, n, N_x, steps) = (500, 20, 50, 100), (2^16, 20, 50, 100), (2^20, 20, 50, 100), with
          and without the trajectory; device events around `--inner` back-to-back launches
  step    the train_nde step of examples/hebb_nde.py (N = 500, affine flow + ToInterval, param_net [50]) three ways:
          graphed (one HIP graph replay per step), eager, and eager with the simulator replaced by the vectorised
          float32 numpy restatement on the host (tests/hebb_restatement.py) -- the path a user had before this kernel:
          device -> host, numpy, host -> device every step

    python tools/hebbbench.py [--reps 20] [--limit 120] [--only kernel|step] [--modes graphed]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "examples"))

import hebb_restatement as H  # noqa: E402
from mogbench import Watchdog  # noqa: E402
from torch_nf_amd import hebb_ops  # noqa: E402
from torch_nf_amd.graphs import GraphedStep  # noqa: E402


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def windows(fn, reps, inner, warmup=3):
    """median, min, max seconds per call of fn over `reps` windows of `inner` calls, after `warmup` windows"""
    times = []
    for r in range(warmup + reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(inner):
            fn()
        end.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(start.elapsed_time(end) * 1e-3 / inner)
    return dict(median_s=float(np.median(times)), min_s=float(min(times)), max_s=float(max(times)))


def host_windows(fn, reps, inner, warmup=3):
    """the same with the host clock around work that ends in a synchronise (steps with host work in them)"""
    times = []
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append((time.perf_counter() - t0) / inner)
    return dict(median_s=float(np.median(times)), min_s=float(min(times)), max_s=float(max(times)))


def kernel_cases(a):
    rng = np.random.RandomState(0)
    n, N_x, steps = 20, 50, 100
    x, w0 = H.inputs(rng, n, N_x)
    xd, wd = f32(x), f32(w0)
    for N, inner in ((500, 200), (1 << 16, 20), (1 << 20, 3)):
        z = f32(H.prior_rows(rng, N))
        for traj in (False, True):
            out = dict(case="kernel", N=N, n=n, N_x=N_x, steps=steps, traj=traj, launches_per_window=inner)
            with Watchdog(a.limit, out):
                t = [0]

                def fn():
                    t[0] += 1
                    return hebb_ops.hebb_simulate(z, xd, wd, steps, 1e-4, seed=1, t=t[0], traj=traj)

                out.update(windows(fn, a.reps, inner))
                sim_steps = N * steps
                out.update(sim_steps_per_s=sim_steps / out["median_s"], ns_per_sim_step=1e9 * out["median_s"] / sim_steps,
                           traj_GBps=(4.0 * sim_steps * n / out["median_s"] / 1e9) if traj else None)
            print(json.dumps(out), flush=True)


def step_cases(a):
    from hebb_nde import build

    N, inner = 500, 50
    results = {}
    for mode in a.modes.split(","):
        system, x0, cde = build(1)
        dev = next(cde.param_net.parameters()).device
        opt = torch.optim.Adam(cde.param_net.parameters(), lr=1e-4, capturable=True)
        params = list(cde.param_net.parameters())
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        x32, w32 = system.x.astype(np.float32), system.w0.astype(np.float32)
        rng = np.random.RandomState(3)

        def simulate(z):
            if mode != "host simulator":
                return system.simulate_device(z, t_dev=counter)
            eps = rng.standard_normal((system.n_steps, N, system.num_neurons)).astype(np.float32)
            w, _ = H.simulate(z.cpu().numpy(), x32, w32, eps, system.sigma_eps, dtype=np.float32)
            return torch.as_tensor(w, device=dev)

        def step():
            z, _ = system.sample_prior_device(N)
            x = simulate(z)
            counter.add_(1)
            loss = -torch.mean(cde.log_prob(z[:, None, :], x))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            for p in params:
                p.grad.clamp_(-1e10, 1e10)
            opt.step()
            return loss.detach()

        out = dict(case="train_nde step", mode=mode, N=N, steps_per_window=inner)
        with Watchdog(a.limit, out):
            if mode == "graphed":
                gs = GraphedStep(step, warmup=3)
                out.update(windows(gs, a.reps, inner))
            elif mode == "eager":
                out.update(host_windows(step, a.reps, inner))
            else:
                out.update(host_windows(step, max(3, a.reps // 4), 5, warmup=1))
            out["final_loss"] = float(step() if mode != "graphed" else gs())
        results[mode] = out["median_s"]
        print(json.dumps(out), flush=True)
    if len(results) == 3:
        print(json.dumps(dict(case="train_nde step, ratios to the host-simulator step",
                              graphed=results["host simulator"] / results["graphed"],
                              eager=results["host simulator"] / results["eager"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds per measurement")
    ap.add_argument("--only", choices=("kernel", "step"))
    ap.add_argument("--modes", default="graphed,eager,host simulator", help="the step's modes, e.g. graphed alone under a profiler")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("hebbbench needs a HIP device: a CPU run says nothing about these times")
    if a.only != "step":
        kernel_cases(a)
    if a.only != "kernel":
        step_cases(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
