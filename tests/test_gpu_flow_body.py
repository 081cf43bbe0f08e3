"""The whole-flow inverse kernel's layer body (flow_fused2.hip / f16_tile2.h) over the paths it takes: D = 64 and 32 and
one padded width (50); S = 4 (layer loop unrolled) and S = 1 (rolled); L = 1, 2, 3; U = 15, 16; N = 1, 31, 33, 4101 (a
partial tile, a partial group, several queue pulls).  z0 and log_prob against oracle/flow_oracle.py in float64, z0 also
against the per-layer route (FUSE_LAYER); one case beyond the f16 operand range (exact re-run) and one row with a NaN.

Bars.  The errors below are the largest over these same cases, measured on the commit before the layer body handed
its split operands from layer to layer (one MI355X, float64 oracle):

    log_prob, |got - want| / max(|want|, 1e-3)             plain and NaN cases 3.034e-07   out-of-range case 3.682e-07
    z0, |got - want| / max(1, largest |z0| of the sample)  plain and NaN cases 6.248e-07   out-of-range case 3.897e-07

The bar is twice that (it was set for a log-det sum that moves from one fp32 association order to another: the
TNF2_LDMFMA build, which measures 3.034e-07 / 3.682e-07 and 6.248e-07 / 3.897e-07, its largest single change 8.0e-08 ->
1.0e-07 in one case).  The shipped body splits where the value is produced and keeps the add chain: every figure is the
parent's.  The distance of z0 to the per-layer route is held to this bar plus the per-layer route's own error against
float64 (triangle inequality), which is measured in the test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARENT_LP_ERR, PARENT_LP_ERR_RANGE = 3.034e-07, 3.682e-07
PARENT_Z0_ERR, PARENT_Z0_ERR_RANGE = 6.248e-07, 3.897e-07
BAR = 2.0

NS = (1, 31, 33, 4101)
CASES = [(D, S, L, (15, 16)[i % 2], NS[i % 4])
         for i, (D, S, L) in enumerate((D, S, L) for D in (64, 32, 50) for S in (4, 1) for L in (1, 2, 3))]


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch_nf_amd


def _flow(tnf, D, S, L, U, N, seed):
    rng = np.random.RandomState(seed)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    params = torch.tensor(rng.normal(0.0, 0.1, (1, nf.D_params))).float()
    mean = torch.tensor(rng.normal(0.0, 0.3, (2 * S, D))).float()
    alpha = torch.tensor(np.exp(rng.normal(0.0, 0.2, (2 * S, D)))).float()
    for b, m, a in zip(nf._bn_layers(), mean, alpha):
        b.set_last_stats(m.cuda(), a.cuda())
    z = torch.tensor(rng.normal(0.0, 1.0, (1, N, D))).float()
    return nf, params, mean, alpha, z


def _truth(oracle, z, params, mean, alpha, D, S, L, U):
    st = [(m.double(), a.double()) for m, a in zip(mean, alpha)]
    z0, _ = oracle.flow_inverse(z.double(), params.double(), D, S, L, U, st)
    return z0, oracle.flow_log_prob(z.double(), params.double(), D, S, L, U, st)


def _whole_flow(tnf, z, params, mean, alpha, D, S, L, U):
    """(log_prob, z0, groups re-run exactly) of the one-launch kernel: D = 2H directly, any other width padded"""
    ops, L_ = tnf.ops, tnf._lib
    with torch.no_grad():
        if D in (32, 64):
            lp, z0, _, re = ops.flow_log_prob_raw(z.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), D, S, L, U, L_.FUSE_FLOW,
                                                  want_z0=True, want_sld=True, count_reruns=True)
        else:
            lp, z0, _, re = ops.flow_padded_log_prob_raw(z.cuda(), params.cuda(), mean.cuda(), alpha.cuda(), D, S, L, U,
                                                         want_z0=True, want_sld=True, count_reruns=True)
    return lp.cpu(), z0.cpu(), int(re.item())


def _per_layer_z0(tnf, nf, z, params):
    nf.fusion = tnf._lib.FUSE_LAYER
    with torch.no_grad():
        z0, _ = nf.inverse_and_log_det(z.cuda(), params.cuda())
    return z0.cpu()


def _lp_err(got, want, rows=None):
    e = (got.double() - want).abs() / want.abs().clamp_min(1e-3)
    return float((e if rows is None else e[:, rows]).max())


def _z0_err(got, want, rows=None):
    e = (got.double() - want.double()).abs() / want.abs().amax(dim=2, keepdim=True).clamp_min(1.0)
    return float((e if rows is None else e[:, rows]).max())


def _check(name, lp, z0, z0_layer, want_lp, want_z0, lp_parent, z0_parent, rows=None):
    e_lp, e_z0 = _lp_err(lp, want_lp, rows), _z0_err(z0, want_z0, rows)
    e_layer, d_layer = _z0_err(z0_layer, want_z0, rows), _z0_err(z0, z0_layer, rows)
    print("FIG %s lp_err %.3e z0_err %.3e z0_layer_err %.3e z0_vs_layer %.3e" % (name, e_lp, e_z0, e_layer, d_layer))
    assert e_lp <= BAR * lp_parent, "%s: log_prob error %.3e > %.3e" % (name, e_lp, BAR * lp_parent)
    assert e_z0 <= BAR * z0_parent, "%s: z0 error %.3e > %.3e" % (name, e_z0, BAR * z0_parent)
    assert d_layer <= BAR * z0_parent + e_layer, "%s: z0 is %.3e from the per-layer route" % (name, d_layer)


@pytest.mark.parametrize("D,S,L,U,N", CASES)
def test_flow_body(tnf, oracle, D, S, L, U, N):
    nf, params, mean, alpha, z = _flow(tnf, D, S, L, U, N, seed=1000 * D + 100 * S + 10 * L + U)
    want_z0, want_lp = _truth(oracle, z, params, mean, alpha, D, S, L, U)
    lp, z0, reruns = _whole_flow(tnf, z, params, mean, alpha, D, S, L, U)
    assert reruns == 0, "%d groups left the fast path" % reruns
    _check("D%d_S%d_L%d_U%d_N%d" % (D, S, L, U, N), lp, z0, _per_layer_z0(tnf, nf, z, params), want_lp, want_z0,
           PARENT_LP_ERR, PARENT_Z0_ERR)


def test_out_of_range_input_takes_the_exact_rerun(tnf, oracle):
    """Samples scaled by 1e5 pass the f16 range of the first layer's operand: every group is detected (the NaN reaches
    the log-det accumulator) and re-run with exact first-layer contractions."""
    D, S, L, U, N = 64, 4, 2, 15, 97
    nf, params, mean, alpha, z = _flow(tnf, D, S, L, U, N, seed=5)
    z = z * 1e5
    want_z0, want_lp = _truth(oracle, z, params, mean, alpha, D, S, L, U)
    assert torch.isfinite(want_lp).all()
    lp, z0, reruns = _whole_flow(tnf, z, params, mean, alpha, D, S, L, U)
    assert reruns > 0, "out-of-range inputs must take the exact path"
    _check("range_z_1e5", lp, z0, _per_layer_z0(tnf, nf, z, params), want_lp, want_z0, PARENT_LP_ERR_RANGE,
           PARENT_Z0_ERR_RANGE)


@pytest.mark.parametrize("D", [64, 50])
def test_row_with_a_nan(tnf, oracle, D):
    """A genuine NaN in one row: that row's log_prob is NaN, as the oracle's is; its group takes the re-run (harmlessly)
    and every other row, the rest of that group included, is as accurate as without it."""
    S, L, U, N, bad = 4, 2, 15, 70, 37
    nf, params, mean, alpha, z = _flow(tnf, D, S, L, U, N, seed=6)
    z[0, bad, 3] = float("nan")       # in the lower half
    z[0, bad, D - 2] = float("nan")   # and in the upper one: both conditioner nets of every layer see it
    want_z0, want_lp = _truth(oracle, z, params, mean, alpha, D, S, L, U)
    rows = torch.arange(N) != bad
    assert torch.isnan(want_lp[0, bad]) and torch.isfinite(want_lp[:, rows]).all()
    lp, z0, reruns = _whole_flow(tnf, z, params, mean, alpha, D, S, L, U)
    assert torch.isnan(lp[0, bad]) and reruns == 1
    _check("nan_row_D%d" % D, lp, z0, _per_layer_z0(tnf, nf, z, params), want_lp, want_z0, PARENT_LP_ERR, PARENT_Z0_ERR, rows)
