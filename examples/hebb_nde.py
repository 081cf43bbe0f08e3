#!/usr/bin/env python3
"""The reference's notebooks/LFI_learning_rules.ipynb (cells 2, 10, 16, 17) on this package: neural density estimation
of the Hebbian learning-rule parameters (alpha, beta, theta_x, b) from the weights after two passes over the inputs,
with an affine flow + ToInterval support layer conditioned through param_net [50].  The simulator runs on the HIP
kernel of include/tnf_hebb.h inside the optimisation step, and each round's step is replayed as one HIP graph.
Usage: python examples/hebb_nde.py --num-iters 200"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd.lfi import train_nde  # noqa: E402
from torch_nf_amd.systems import HebbLearn  # noqa: E402


def build(rs=1, num_neurons=20, N_x=50):
    """(system, x0, cde) of the notebook's cell 17 configuration."""
    np.random.seed(rs)
    torch.manual_seed(rs)
    system = HebbLearn(num_neurons, N_x)
    x0 = system.simulate(np.array([[0.02, 0.00, 0.0, 10.0]]), t=0)  # cell 10: the data distribution's parameters
    nf = tnf.NormFlow(system.D, True, "affine", support_layer=system.support_layer)
    cde = tnf.ConditionalDensityEstimator(nf, x0.shape[1], [50])
    return system, x0, cde


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rs", type=int, default=1)
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--num-iters", type=int, default=2000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--eager", action="store_true")
    args = ap.parse_args()
    system, x0, cde = build(args.rs)
    t0 = time.time()
    losses = train_nde(cde, system, x0, N=args.N, R=args.R, num_iters=args.num_iters, lr=1e-4, clip=1e10,
                       use_graph=False if args.eager else None, verbose=True)
    dt = time.time() - t0
    print("%.3f ms per iteration (%d simulations of %d steps each); final loss %.3f"
          % (1e3 * dt / len(losses), args.N, system.n_steps, float(np.mean(losses[-50:]))))
    dev = next(cde.param_net.parameters()).device
    with torch.no_grad():
        z, _ = cde.sample(torch.as_tensor(x0, dtype=torch.float32, device=dev), N=1000)
    print("posterior mean (alpha, beta, theta_x, b):", z[0].mean(0).cpu().numpy(), " data generated at [0.02 0 0 10]")
