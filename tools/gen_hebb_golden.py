"""Generate tests/golden/hebb.npz by RUNNING THE REFERENCE's `hebb` (notebooks/LFI_learning_rules.ipynb, cell 8) --
development machine only; no test runs this script.

Usage:  python3 tools/gen_hebb_golden.py <checkout of the reference>/notebooks/LFI_learning_rules.ipynb

The notebook's JSON is loaded, the source of cell 8 is exec'd in a namespace this script fills with `np`, `x` and
`num_neurons`, and the function it defines is called.  The cell draws `w0` and sets `sigma_eps` when it runs: w0 is
read back, rounded to float32 (so that the kernel sees exactly the reference's starting state) and put back into the
namespace before the calls; sigma_eps is read back.  Nothing of the notebook's text is stored anywhere.

The fixture (plain float64 arrays, < 100 KB):
    x (50, 20), w0 (20,), z (32, 4)   float32-exact values; z rows 0 .. 23 from the benign box of the tests (alpha, beta
                                      log-uniform on [1e-5, 1e-2], theta_x in (-3, 3), b in (1, 20)), rows 24 .. 31 from
                                      the whole prior (alpha, beta up to 1e-1)
    sigma_eps ()                      the cell's value
    noise_seed ()                     np.random.seed in force at each call: the call's noise is, step by step,
                                      sigma_eps * np.random.normal(0, 1, (32, 20)), 100 draws
    steps (5,)                        0, 1, 49, 50, 99
    traj (5, 32, 20)                  hebb(z, traj=True) at those steps
    w_final (32, 20)                  hebb(z, traj=False) under the same seed
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hebb_restatement as H  # noqa: E402  (the groups' parameter draws, shared with the tests)

OUT = os.path.join(ROOT, "tests", "golden", "hebb.npz")
N_NEURONS, N_X, INPUT_SEED, NOISE_SEED = 20, 50, 20260, 8
STEPS = np.array([0, 1, 49, 50, 99])


def f32_exact(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1]) as f:
        cells = json.load(f)["cells"]
    src = "".join(cells[8]["source"])
    rng = np.random.RandomState(INPUT_SEED)
    x, _ = H.inputs(rng, N_NEURONS, N_X)
    x = f32_exact(x)
    z = f32_exact(np.concatenate((H.prior_rows(rng, 24, "box"), H.prior_rows(rng, 8))))
    ns = {"np": np, "x": x, "num_neurons": N_NEURONS}
    np.random.seed(INPUT_SEED + 1)
    exec(compile(src, "cell8", "exec"), ns)
    assert callable(ns.get("hebb")) and "w0" in ns and "sigma_eps" in ns, "cell 8 is not the simulator's cell"
    ns["w0"] = f32_exact(ns["w0"])
    sigma_eps = float(ns["sigma_eps"])
    np.random.seed(NOISE_SEED)
    traj = np.asarray(ns["hebb"](z.copy(), traj=True), dtype=np.float64)
    np.random.seed(NOISE_SEED)
    w_final = np.asarray(ns["hebb"](z.copy(), traj=False), dtype=np.float64)
    assert traj.shape == (2 * N_X, 32, N_NEURONS) and np.array_equal(traj[-1], w_final) and np.isfinite(traj).all()
    np.savez_compressed(OUT, x=x, w0=ns["w0"], z=z, sigma_eps=np.float64(sigma_eps), noise_seed=np.int64(NOISE_SEED),
                        steps=STEPS, traj=traj[STEPS], w_final=w_final)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
