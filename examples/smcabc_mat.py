#!/usr/bin/env python3
"""The reference's scripts/smcabc_mat.py on this package: the ABC-SMC baseline of the LFI comparison on the matrix
det/trace simulator, all rounds of all particles in one HIP kernel launch.  Same arguments and the same output file
fields (zs, xs, time_per_samp); --N is added (the script fixes N = 50).  The script's statistics are (trace, det):
T_x0 = [d/2, 0], tolerances [2, d/2] -> [0.02, 2]; this package's Mat orders them (det, trace), so the same schedule is
applied in that order.  Usage: python examples/smcabc_mat.py --d 2 --T 50"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_nf_amd.lfi import ABC_SMC  # noqa: E402
from torch_nf_amd.systems import GaussianProposal, Mat  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--d", type=int, default=2)
ap.add_argument("--T", type=int, default=50)
ap.add_argument("--sigma", type=float, default=0.25)
ap.add_argument("--rs", type=int, default=1)
ap.add_argument("--N", type=int, default=50)
args = ap.parse_args()
d, T, sigma, rs, N = args.d, args.T, args.sigma, args.rs, args.N
np.random.seed(rs)

mat = Mat(d)
T_x0 = np.array([[0.0, d / 2]])  # det = 0, trace = d / 2
proposal = GaussianProposal(sigma ** 2 * np.eye(mat.D), mat.lb, mat.ub)
eps1, epsT = [d / 2, 2.0], [2.0, 0.02]  # (det, trace): the script's [2, d/2] -> [0.02, 2] in its (trace, det) order
all_eps = np.stack([np.linspace(eps1[i], epsT[i], T) for i in range(2)], axis=1)

time0 = time.time()
zs = ABC_SMC(N, mat, proposal, T_x0, all_eps)

fname = "SMCABC_mat_d=%d_T=%d_sigma=%.2e_rs=%d.npz" % (d, T, sigma, rs)
if zs is not None:
    time_per_samp = (time.time() - time0) / N
    print(zs.shape)
    xs = mat.simulate(zs[-1])
    np.savez(fname, zs=zs, xs=xs, time_per_samp=time_per_samp)
    print("%.3e s per sample; final statistics: mean" % time_per_samp, xs.mean(0), "std", xs.std(0), "target", T_x0[0])
else:
    np.savez(fname, zs=0, xs=0, time_per_samp=np.nan)
    print("a particle used up its candidates in one round: no samples (the script's `zs is None` branch)")
