"""Time the MoG kernels (one GPU process; every step under its own time limit: a watchdog thread ends the process with
status 124 when a step overruns -- a thread, because a signal handler cannot interrupt a blocked synchronize):

  lane    log_prob and forward + backward at (M = 2^16, N = 1, D = 5, K = 5): a parameter row per context, one lane each
  shared  log_prob and forward + backward at (M = 1, N = 2^20, D = 5, K = 5): one shared row
  sample  the sampling kernel at both shapes

Each line reports the kernel time, the fraction of the compulsory-HBM-byte roof it reaches (for N = 1:
(D_params + D + 1) * 4 B per context; `--hbm-gbs` is the streaming rate taken as the roof) and the ratio to the same
formula written in torch ops on the GPU (`torch_ops_log_prob` below: it forms Sigma_inv, as the reference does).

    python tools/mogbench.py [--steps 50] [--warmup 10] [--limit 60] [--hbm-gbs 4000]
"""
import argparse
import json
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torch_nf_amd.density_estimator import MoG  # noqa: E402

EPS = 1e-12


def torch_ops_log_prob(mog, z, params):
    """The reference's formula as a composition of torch ops (unbounded, K > 1)."""
    alpha, mu, Sigma_inv, Sigma_det = mog._get_MoG_params(params)
    d = z[:, :, None, :] - mu[:, None, :, :]
    q = torch.matmul(torch.matmul(d[:, :, :, None, :], Sigma_inv[:, None]), d[:, :, :, :, None])[:, :, :, 0, 0]
    den = torch.sqrt(((2 * np.pi) ** mog.D) * Sigma_det + EPS)[:, None, :]
    return torch.log(torch.sum(alpha[:, None, :] * torch.exp(-0.5 * q) / den, dim=2) + EPS)


class Watchdog(object):
    """`with Watchdog(seconds, what)`: ends the process (status 124) if the block runs longer."""

    def __init__(self, seconds, what):
        self.timer = threading.Timer(seconds, self._expire, [seconds, what])
        self.timer.daemon = True

    def _expire(self, seconds, what):
        print(json.dumps(dict(what, error="time limit of %d s" % seconds)), flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e-3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=60, help="seconds per step")
    ap.add_argument("--hbm-gbs", type=float, default=4000.0)
    a = ap.parse_args()
    D, K = 5, 5
    mog = MoG(D, True, K)
    P = mog.D_params
    rng = np.random.RandomState(0)
    for name, M, N in (("lane", 1 << 16, 1), ("shared", 1, 1 << 20)):
        p = torch.tensor(0.3 * rng.normal(0, 1, (M, P))).float().cuda()
        with torch.no_grad():
            mu = mog._get_MoG_params(p)[1]
        z = (mu[:, :1, :] + 0.3 * torch.randn(M, N, D, device="cuda")).contiguous()
        pg = p.clone().requires_grad_()
        g = torch.randn(M, N, device="cuda")
        u, e1, e2 = torch.rand(M, N, device="cuda"), torch.randn(M, N, D, device="cuda"), torch.randn(M, N, D, device="cuda")

        def fwd():
            with torch.no_grad():
                return mog.log_prob(z, p)

        def fwd_bwd():
            return torch.autograd.grad(mog.log_prob(z, pg), [pg], g)

        def ref_fwd():
            with torch.no_grad():
                return torch_ops_log_prob(mog, z, p)

        def ref_fwd_bwd():
            return torch.autograd.grad(torch_ops_log_prob(mog, z, pg), [pg], g)

        def sample():
            return mog._forward_from(u, e1, e2, p)

        rows = M if N == 1 else 1
        fwd_bytes = rows * P * 4 + M * N * (D + 1) * 4
        steps = {"log_prob": (fwd, ref_fwd, fwd_bytes), "fwd_bwd": (fwd_bwd, ref_fwd_bwd, 2 * fwd_bytes + rows * P * 4),
                 "sample": (sample, None, rows * P * 4 + M * N * (3 * D + 2) * 4)}
        for step, (fn, ref, nbytes) in steps.items():
            out = {"layout": name, "step": step, "M": M, "N": N, "D": D, "K": K}
            with Watchdog(a.limit, out):
                t = timed(fn, a.steps, a.warmup)
                out.update(seconds=t, samples_per_s=M * N / t, roof_fraction=nbytes / (a.hbm_gbs * 1e9) / t)
                if ref is not None:
                    out["torch_ops_ratio"] = timed(ref, max(1, a.steps // 10), 2) / t
            print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
