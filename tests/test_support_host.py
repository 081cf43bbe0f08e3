"""The host half of the support-layer sweep (tests/test_gpu_support_domain.py), no GPU: the noise model of its bars.

The standalone bars are 4 x the float32 oracle's error against the float64 oracle; the fused bars add 4 x the absolute
error of interval_fast (csrc/support_math.h) restated in float32 (tests/support_restatement.py).  Here: both noise
figures sit in the guard 1e-9 .. 1e-5 over the sweep's inputs, the restated launcher tiling is consistent, and the sweep
bites -- one flipped sign or one swapped pair of constant rows in the restatement lands outside 4 x the oracle noise."""
import pytest
import torch

import support_restatement as SR
from domain_helpers import float64

HOST_D = (1, 2, 3, 5, 17, 21, 31, 32, 33, 64, 127, 257, 1000)
ROWS = 40


@pytest.fixture(scope="module")
def cases(oracle):
    out = [SR.IntervalCase(oracle, D, "mixed", ROWS) for D in HOST_D]
    return out + [SR.IntervalCase(oracle, D, p, ROWS) for D in (5, 33) for p in SR.KINDS]


def _restated_err(c, oracle, inverse, **defect):
    """(values, log-dets) of the restatement against the float64 oracle in the sweep's measure."""
    inp = c.x if inverse else c.z
    out, ld = SR.restated(inp, c.c7, inverse, **defect)
    want, want_ld, _ = c.ref64[inverse]
    return SR.err(out, want), SR.err(ld, want_ld)


def test_oracle_noise_within_guard(cases):
    v = max(c.noise()[0] for c in cases)
    g = max(c.noise()[1] for c in cases)
    print("float32 oracle noise: values and log-dets %.3e, gradients %.3e" % (v, g))
    assert 1e-9 < v < 1e-5 and 1e-9 < g < 1e-5


def test_simplex_oracle_noise_within_guard(oracle):
    cs = [SR.SimplexCase(oracle, Din, Din + a, ROWS) for Din in HOST_D for a in (0, 1)]
    v, g = max(c.noise()[0] for c in cs), max(c.noise()[1] for c in cs)
    print("float32 oracle noise, ToSimplex: values and log-dets %.3e, gradients %.3e" % (v, g))
    assert 1e-9 < v < 1e-5 and 1e-9 < g < 1e-5
    for c in cs:
        assert float(c.ref64[0][..., -1].min()) >= 1e-3  # the last output stays off the 1e-10 floor of the log-det


def test_restatement_agrees_with_the_float64_oracle(cases, oracle):
    worst = max(max(_restated_err(c, oracle, inverse)) for c in cases for inverse in (False, True))
    print("interval_fast restated in float32 against the float64 oracle: %.3e" % worst)
    assert 1e-9 < worst < 1e-5


def test_identity_features_pass_through(cases):
    for c in cases:
        idt = c.kind == 3
        for inverse in (False, True):
            inp = c.x if inverse else c.z
            out, _ = SR.interval_fast_restated(inp.numpy(), c.c7.numpy(), inverse)
            assert torch.equal(torch.from_numpy(out)[..., idt], inp[..., idt])
        if c.pattern == "identity":
            assert float(c.ref64[False][1].abs().max()) == 0.0


@pytest.mark.parametrize("defect", [dict(flip_sign=True), dict(permute_rows=(2, 3)), dict(permute_rows=(4, 5)),
                                    dict(permute_rows=(0, 1))], ids=["sign", "tanh_m-tanh_c", "softplus_m-softplus_c", "flags"])
def test_the_sweep_bites(cases, oracle, defect):
    """A planted defect in the restatement -- the formulas the fused kernels run -- is far outside the standalone bar
    (4 x the float32 oracle's noise) in both directions on every mixed case that has the feature kind it touches."""
    bar = 4.0 * max(c.noise()[0] for c in cases)
    for c in cases:
        if c.pattern != "mixed" or c.D < 3:
            continue
        for inverse in (False, True):
            assert max(_restated_err(c, oracle, inverse)) <= bar  # sound as it stands ...
            e = max(_restated_err(c, oracle, inverse, **defect))
            assert not e <= bar, (c.D, inverse, defect, e, bar)  # ... and caught with the defect (NaN counts as caught)


def test_launcher_tiling_restated():
    """rows_per_block and the 64 KB refusal of support_kernels.hip: R = 256 for narrow rows, 1 from D = 5000 on in both
    dtypes, the accepted limits, and every block of every sweep case within the 64 KB."""
    assert SR.rows_per_block(1, 4, 1) == 256 and SR.rows_per_block(31, 4, 1) == 256 and SR.rows_per_block(32, 4, 1) == 248
    assert SR.rows_per_block(5000, 4, 1) == SR.rows_per_block(5000, 8, 1) == 1
    assert SR.rows_per_block(5000, 4, 3) == SR.rows_per_block(5000, 8, 3) == 1
    assert [SR.max_width(e, b) for e in (4, 8) for b in (False, True)] == [16383, 8190, 8191, 4094]
    for D in SR.D_LIST:
        for esz in (4, 8):
            assert SR.lds_bytes(D, esz, False) <= SR.LDS_LIMIT
            # the one sweep case past a limit: ToSimplex backward, float64, Din = 5000 > 4094 (the sweep asserts the refusal)
            assert (SR.lds_bytes(D, esz, True) <= SR.LDS_LIMIT) == ((D, esz) != (5000, 8))
    assert SR.row_edges(1) == [1, 2, 3] and SR.row_edges(256) == [1, 255, 256, 257, 513]


def test_float64_context_restores_the_default():
    with float64():
        assert torch.get_default_dtype() == torch.float64
    assert torch.get_default_dtype() == torch.float32
