#!/usr/bin/env python3
"""The reference's notebooks/two_network_arch.ipynb (cells 2, 5, 6) on this package: an exponential family network for
the Dirichlet family, D = 5 -- a coupling flow on R^4 behind a ToSimplex support layer, conditioned on the natural
parameter eta through param_net [100], M = N = 100.  The whole iteration (prior draw, sampling, loss, backward, Adam, KL)
runs on the device (efn.train_efn, include/tnf_efn.h) and is replayed as one HIP graph.
Usage: python examples/efn_dirichlet.py --num-iters 2000"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd.efn import train_efn  # noqa: E402


def build(rs=4, D=5):
    """(exp_fam, cde) of the notebook's cell 6 configuration."""
    np.random.seed(rs)
    torch.manual_seed(rs)
    exp_fam = tnf.Dirichlet(D)
    nf = tnf.NormFlow(D - 1, True, "coupling", 1, 1, 15, support_layer=tnf.ToSimplex(D - 1))
    return exp_fam, tnf.ConditionalDensityEstimator(nf, exp_fam.D_eta, [100])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rs", type=int, default=4)
    ap.add_argument("--M", type=int, default=100)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--num-iters", type=int, default=2000)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    exp_fam, cde = build(args.rs)
    t0 = time.time()
    losses, KLs = train_efn(cde, exp_fam, M=args.M, N=args.N, num_iters=args.num_iters, lr=1e-4, seed=args.rs,
                            use_graph=False if args.eager else None, verbose=True)
    dt = time.time() - t0
    q = max(1, len(losses) // 10)
    print("%d iterations, %.3f ms each; loss %.4f -> %.4f, KL %.4f -> %.4f (means of the first and last tenth)"
          % (len(losses), 1e3 * dt / max(1, len(losses)), losses[:q].mean(), losses[-q:].mean(), KLs[:q].mean(),
             KLs[-q:].mean()))
