"""Generate tests/golden/mog.npz by RUNNING THE REFERENCE's torch_nf.density_estimator.MoG (development machine only; it
needs scipy, which the reference imports -- no test runs this script).

Usage (cwd outside this repo so nothing shadows the reference's namespace package):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<checkout of the reference> \
        python3 <this repo>/tools/gen_mog_golden.py

Cases (D, K) in {(2,1), (2,3), (5,1), (5,4), (8,2), (16,1)}, each without ("u") and with ("b") bounds, M = 3, N = 7,
under the prefix "d<D>k<K><u|b>_":
    params (3, D_params), z (3, 7, D)   float32: params ~ 0.5 N(0, 1); z = a component mean + 0.5 N(0, 1), so that
                                        the density is far above the EPS floor (asserted: every lp64 > -20 for K > 1)
    lb, ub (D,)                         float64 multiples of 1/8 (exact in float32), bounded cases only
    alpha, mu, Sigma_inv, Sigma_det     the reference's _get_MoG_params(params), float32
    lp32 (3, 7)                         the reference's log_prob as it runs (float32)
    lp64 (3, 7), g_lp (3, 7), g_params  the same under torch.set_default_dtype(torch.float64) on the float64 copies of
                                        the same inputs, and its autograd gradient of sum(g_lp * lp64)
One more case, "floor_" (D = 16, K = 2, unbounded), lies deliberately on the floor: z far from every mean.
Plain arrays only.  The reference is imported and called; no source text of it is stored anywhere.
"""
import os

import numpy as np
import torch

import torch_nf.density_estimator as ref  # the reference (PYTHONPATH=<checkout of the reference>)

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "mog.npz")
assert not os.path.abspath(ref.__file__).startswith(os.path.dirname(HERE) + os.sep), ref.__file__
torch.set_num_threads(1)
M, N = 3, 7


def case(out, key, D, K, bounded, spread):
    rng = np.random.RandomState(7000 + 100 * D + 10 * K + int(bounded) + (5 if spread > 1 else 0))
    lb = ub = None
    if bounded:
        lb = -np.round(8 * rng.uniform(1.0, 3.0, D)) / 8.0
        ub = np.round(8 * rng.uniform(1.5, 4.0, D)) / 8.0
        out[key + "lb"], out[key + "ub"] = lb, ub
    mog = ref.MoG(D, True, K, lb, ub)
    params = (0.5 * rng.normal(0.0, 1.0, (M, mog.D_params))).astype(np.float32)
    p32 = torch.tensor(params)
    alpha, mu, Sigma_inv, Sigma_det = mog._get_MoG_params(p32)
    comp = rng.randint(0, K, (M, N))
    z = mu.numpy()[np.arange(M)[:, None], comp] + spread * rng.normal(0.0, 1.0, (M, N, D))
    z = z.astype(np.float32)
    out[key + "params"], out[key + "z"] = params, z
    out[key + "alpha"], out[key + "mu"] = alpha.numpy(), mu.numpy()
    out[key + "Sigma_inv"], out[key + "Sigma_det"] = Sigma_inv.numpy(), Sigma_det.numpy()
    lp32 = mog.log_prob(torch.tensor(z), p32)
    assert lp32.dtype == torch.float32 and tuple(lp32.shape) == (M, N)
    out[key + "lp32"] = lp32.numpy()
    torch.set_default_dtype(torch.float64)
    try:
        p64 = torch.tensor(params.astype(np.float64), requires_grad=True)
        lp64 = mog.log_prob(torch.tensor(z.astype(np.float64)), p64)
        assert lp64.dtype == torch.float64
        g_lp = rng.normal(0.0, 1.0, (M, N))
        (g_params,) = torch.autograd.grad((lp64 * torch.tensor(g_lp)).sum(), p64)
    finally:
        torch.set_default_dtype(torch.float32)
    out[key + "lp64"], out[key + "g_lp"], out[key + "g_params"] = lp64.detach().numpy(), g_lp, g_params.numpy()
    return out[key + "lp64"]


def main():
    out = {}
    for D, K in ((2, 1), (2, 3), (5, 1), (5, 4), (8, 2), (16, 1)):
        for bounded in (False, True):
            lp64 = case(out, "d%dk%d%s_" % (D, K, "b" if bounded else "u"), D, K, bounded, 0.5)
            assert np.all(np.isfinite(lp64))
            if K > 1:
                assert lp64.min() > -20.0, (D, K, bounded, lp64.min())  # meaningful inputs: off the EPS floor
    lp64 = case(out, "floor_", 16, 2, False, 6.0)
    assert np.all(np.abs(lp64 - np.log(1e-12)) < 1e-9), lp64
    for v in out.values():
        assert isinstance(v, np.ndarray) and v.dtype in (np.float64, np.float32)
    np.savez_compressed(OUT, **out)
    with np.load(OUT, allow_pickle=False) as f:
        assert sorted(f.files) == sorted(out) and all(np.array_equal(f[n], out[n]) for n in out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
