"""Generate tests/golden/expfam.npz by RUNNING THE REFERENCE's torch_nf.exponential_families (development machine only;
it needs scipy, which the reference imports -- this script is the only place scipy is needed, no test runs it).

Usage (cwd outside this repo so nothing shadows the reference's namespace package):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<checkout of the reference> \
        python3 <this repo>/tools/gen_expfam_golden.py

For D in {2, 5, 20} and both families the fixture records, under the prefix "<mvn|dir><D>_":
    eta            (5, D_eta)  the reference's sample_eta(5) under np.random.seed
    mu, Sigma / alpha          eta_to_mu(eta);   eta_rt = mu_to_eta(...) of those (the round trip)
    z64, z32       (3, 7, D)   MVN: z ~ N(0, 10), Dirichlet: z ~ U[0.1, 3], as in the reference's own test
    T64, T32       (3, 7, D_eta) the reference's T(z)
    dot64, dot32   (3, 7)      eta . T(z) the reference's way: matmul(T(z), eta[:3, :, None]) in z's dtype
    lp, KL         (3, 7), (3,)  a log_prob array and the reference's KL(z64, lp, eta[:3])
Plain arrays only.  The reference is imported and called; no source text of it is stored anywhere.
"""
import os

import numpy as np
import torch

import torch_nf.exponential_families as ref  # the reference (PYTHONPATH=<checkout of the reference>)

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "expfam.npz")
assert not os.path.abspath(ref.__file__).startswith(os.path.dirname(HERE) + os.sep), ref.__file__
torch.set_num_threads(1)


def main():
    out = {}
    for name, cls in (("mvn", ref.MVN), ("dir", ref.Dirichlet)):
        for D in (2, 5, 20):
            fam = cls(D)
            k = "%s%d_" % (name, D)
            np.random.seed(1000 + D + (0 if name == "mvn" else 100))
            eta = fam.sample_eta(5)
            assert eta.shape == (5, fam.D_eta) and eta.dtype == np.float64
            out[k + "eta"] = eta
            if name == "mvn":
                mu, Sigma = fam.eta_to_mu(eta)
                out[k + "mu"], out[k + "Sigma"] = mu, Sigma
                out[k + "eta_rt"] = fam.mu_to_eta(mu, Sigma)
                z = np.random.normal(0.0, 10.0, (3, 7, D))
            else:
                alpha = fam.eta_to_mu(eta)
                out[k + "alpha"] = np.array(alpha)
                out[k + "eta_rt"] = fam.mu_to_eta(alpha)
                z = np.random.uniform(0.1, 3.0, (3, 7, D))
            for tag, dt in (("64", torch.float64), ("32", torch.float32)):
                zt = torch.tensor(z, dtype=dt)
                T = fam.T(zt)
                assert T.dtype == dt and tuple(T.shape) == (3, 7, fam.D_eta)
                dot = torch.matmul(T, torch.tensor(eta[:3], dtype=dt)[:, :, None])[:, :, 0]
                out[k + "z" + tag] = zt.numpy()
                out[k + "T" + tag] = T.numpy()
                out[k + "dot" + tag] = dot.numpy()
                assert np.array_equal(out[k + "T" + tag], fam.T(torch.tensor(out[k + "z" + tag])).numpy())
            lp = np.random.normal(0.0, 1.0, (3, 7))
            out[k + "lp"] = lp
            out[k + "KL"] = fam.KL(out[k + "z64"], lp, eta[:3])
            assert out[k + "KL"].shape == (3,) and np.all(np.isfinite(out[k + "KL"]))
    for v in out.values():
        assert isinstance(v, np.ndarray) and v.dtype in (np.float64, np.float32)
    np.savez_compressed(OUT, **out)
    with np.load(OUT, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(out) and all(np.array_equal(f[n], out[n]) for n in out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
