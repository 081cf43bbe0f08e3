"""The host half of the MAF sweep (tests/test_gpu_maf_domain.py), no GPU: what licenses its bars and its case names.

The sweep's bars are 4 x the float32 error of the matrix-pipe formulation restated in torch (tests/maf_restatement.py:
folded_maf and the AR fold around it) against the float64 oracle.  Here: in float64 that restatement IS the oracle's
function (values to 1e-12, autograd gradients to 1e-11, padded to the kernels' 16-multiples or not) and three planted
defects break that; the restated LDS bounds reproduce the library's answers over the whole domain, so the restated nacc
names each case's accumulator scheme; the sweep's grid, evaluated with those formulas, reaches every instantiation; and
the float32 noise of every group is above rounding to nothing and, times 4, inside the constants the suite used so far."""
import ctypes

import pytest
import torch

import maf_restatement as MR
from domain_helpers import float64

PIN_SHAPES = [(4, 1, 20), (16, 3, 17), (33, 2, 40), (21, 2, 42)]  # L = 1; padded D and U (33 -> 48, 40 -> 48; 21, 42)


@pytest.fixture(scope="module")
def tnf():
    import torch_nf_amd

    return torch_nf_amd


@pytest.fixture(scope="module")
def sweep(tnf, oracle):
    s = MR.Sweep(tnf, oracle)
    for section in MR.SECTIONS:
        s.need(section)
    return s


def _pin(tnf, oracle, D, L, U, **kw):
    """(value error, gradient error) of folded_maf against oracle.maf in float64, the larger of the two directions."""
    c = MR.MafCase(tnf, oracle, D, L, U, rows=(3, 9))
    g = torch.Generator().manual_seed(D)
    wz, wl = torch.randn(3, 9, D, generator=g), torch.randn(3, 9, generator=g)
    v = gr = 0.0
    with float64():
        for inverse in (True, False):
            want = c.oracle.maf(c.z.double(), c.params.double(), D, L, U, c.Ms, inverse)
            got = MR.folded_maf(c.z.double(), c.params.double(), D, L, U, c.Ms, inverse, **kw)
            assert got[0].dtype == got[1].dtype == torch.float64
            v = max(v, MR.err(got[0], want[0]), MR.err(got[1], want[1]))
            gw = MR.maf_grads(lambda z, p: oracle.maf(z, p, D, L, U, c.Ms, inverse), c.z, c.params, wz, wl, torch.float64)
            gg = MR.maf_grads(lambda z, p: MR.folded_maf(z, p, D, L, U, c.Ms, inverse, **kw), c.z, c.params, wz, wl, torch.float64)
            gr = max(gr, MR.gerr(gg[0], gw[0]), MR.gerr(gg[1], gw[1]))
    return v, gr


@pytest.mark.parametrize("pad", [False, True], ids=["exact", "padded"])
@pytest.mark.parametrize("D,L,U", PIN_SHAPES, ids=[MR.case_id(*s) for s in PIN_SHAPES])
def test_folded_maf_is_the_oracles_function(tnf, oracle, D, L, U, pad):
    v, g = _pin(tnf, oracle, D, L, U, pad=pad)
    print("folded_maf against oracle.maf in float64, D%d L%d U%d pad=%d: values %.2e, gradients %.2e" % (D, L, U, pad, v, g))
    assert v <= 1e-12 and g <= 1e-11


@pytest.mark.parametrize("defect", [dict(drop_seed=1), dict(drop_seed=2), dict(pad=True, half_fold=True)],
                         ids=["hidden-seed", "output-seed", "half-fold"])
def test_the_pin_bites(tnf, oracle, defect):
    """A dropped column-sum seed of the hidden or of the output layer, or -c instead of -2 c folded into the weights that
    consume r, is far outside the pin."""
    D, L, U = 33, 2, 40
    v, g = _pin(tnf, oracle, D, L, U, **defect)
    print("planted %s: values %.2e, gradients %.2e" % (defect, v, g))
    assert v > 1e-9 and g > 1e-9


def test_ar_fold_is_the_oracles_function(tnf, oracle):
    for D, L, U in [(5, 1, 15), (21, 2, 42), (33, 3, 17)]:
        c = MR.ArCase(tnf, oracle, D, L, U, rows=(3, 9))
        a = (D, L, U, c.Ms)
        with float64(), torch.no_grad():
            st, p, z = tuple(s.double() for s in c.stat), c.params.double(), c.z.double()
            for Mp in (3, 1):
                want = MR.oracle_ar_inverse(oracle, z, p[:Mp], *a, st) + MR.oracle_ar_forward(oracle, z, p[:Mp], *a, st)
                got = MR.folded_ar_log_prob(z, p[:Mp], *a, st) + MR.folded_ar_forward(z, p[:Mp], *a, st)
                assert torch.equal(want[0], oracle.ar_flow_log_prob(z, p[:Mp], *a, st))
                for g_, w_ in zip(got, want):
                    assert g_.dtype == torch.float64 and MR.err(g_, w_) <= 1e-12


def test_lds_limits_restated():
    """The restated formulas against tnf_ar_flow_supported / tnf_ar_flow_train_supported over the whole domain (the
    library is loaded as tests/test_cabi.py does); the refused forward cells are exactly the four named."""
    from torch_nf_amd import _lib

    raw = ctypes.CDLL(_lib.LIB_PATH)
    refused = set()
    for D in range(1, 65):
        for L in range(1, 6):
            for U in range(1, 65):
                assert bool(raw.tnf_ar_flow_supported(D, L, U)) == MR.fwd_supported(D, L, U), (D, L, U)
                assert bool(raw.tnf_ar_flow_train_supported(D, L, U)) == MR.train_supported(D, L, U), (D, L, U)
                if not MR.fwd_supported(D, L, U):
                    refused.add((MR.tiles(D, U)[0], L, MR.tiles(D, U)[1]))
    assert sorted(refused) == sorted(MR.UNSUPPORTED_FWD)
    assert not raw.tnf_ar_flow_supported(65, 1, 16) and not raw.tnf_ar_flow_supported(16, 6, 16)
    assert not raw.tnf_ar_flow_supported(16, 1, 65) and not raw.tnf_ar_flow_train_supported(33, 1, 16)
    # the fused backward's cell of tests/test_gpu_maf.py: one shared accumulator copy, hence fixed point
    assert MR.nacc(21, 2, 42) == 1 and MR.nacc(6, 2, 15) == 4


def test_launch_geometry_restated():
    assert MR.fwd_bx(277, 512) == 4 and MR.tiles_per_wave(277, 4) == 2      # 18 tiles on 16 waves: a second, ragged tile
    assert MR.fwd_bx(277, 1) == 5 and MR.fwd_bx(1 << 20, 1) == 2048 and MR.fwd_bx(65, 3) == 2
    assert MR.bwd_bx(147, 3) == 1 and MR.tiles_per_wave(147, 1) == 3        # one workgroup walks 10 tiles
    assert MR.bwd_bx(37, 1) == 1 and MR.bwd_bx(147, 1) == 3
    assert MR.adds_fbits(37, 1) == (3, 16) and MR.adds_fbits(147, 3) == (10, 14)
    # the smallest N at which the 512-workgroup cap binds: 2,050 tiles, 5 terms per accumulator, one fraction bit fewer
    assert MR.bwd_bx(MR.LONG_N - 21, 1) == 512 and MR.adds_fbits(MR.LONG_N - 21, 1) == (4, 16)
    assert MR.bwd_bx(MR.LONG_N, 1) == 512 and MR.adds_fbits(MR.LONG_N, 1) == (5, 15)
    assert MR.tiles_per_wave(MR.LONG_N, 512) == 2
    assert [MR.train_mode(*s) for s in MR.LONG_CELLS] == ["fixed", "private"]
    assert all(MR.train_supported(*s) for s in MR.LONG_CELLS)


def test_grid_reaches_every_instantiation():
    """The GPU grid, evaluated host-side.  Forward: every supported (DT, UT, INV, VEC) -- both directions run on every
    shape, so (DT, UT, VEC); the four refused cells appear as routes to the generic kernel.  Backward, plain mode: every
    supported (DT, UT, VEC) x the nacc values that cell has over L = 1 .. 3; fused mode: every supported (DT, UT) x nacc;
    the refused backward cells appear as routes to the generic kernel."""
    def vec(D):
        return D % 4 == 0

    domain = [(D, L, U) for D in range(2, 65) for L in range(1, 6) for U in range(5, 65)]
    # forward
    grid = [s for DT in MR.DTS for UT in MR.UTS for s in MR.forward_cell(DT, UT)] + [MR.walk_shape(DT) for DT in MR.DTS]
    want = {(*MR.tiles(D, U), vec(D)) for D, L, U in domain if MR.fwd_supported(D, L, U)}
    got = {(*MR.tiles(D, U), vec(D)) for D, L, U in grid if MR.fwd_supported(D, L, U)}
    assert got == want and len(want) == 32
    refused = {(MR.tiles(D, U)[0], L, MR.tiles(D, U)[1]) for D, L, U in grid if not MR.fwd_supported(D, L, U)}
    assert sorted(refused) == sorted(MR.UNSUPPORTED_FWD)
    for DT in MR.DTS:
        for UT in MR.UTS:
            Ls = {L for D, L, U in MR.forward_cell(DT, UT)}
            assert {1, 2, 3} <= Ls and max(L for L in range(1, 6) if MR.fwd_supported(16 * DT, L, 16 * UT)) in Ls
    ar = [s for DT in MR.DTS for UT in MR.UTS for s in MR.ar_cell(DT, UT)]
    assert all(MR.fwd_supported(*s) for s in ar) and {MR.tiles(D, U) for D, L, U in ar} == {(a, b) for a in MR.DTS for b in MR.UTS}
    # backward, plain mode
    plain = MR.backward_cases()
    want = {(*MR.tiles(D, U), vec(D), MR.nacc(D, L, U)) for D, L, U in domain if MR.bwd_supported(D, L, U)}
    got = {(*MR.tiles(D, U), vec(D), MR.nacc(D, L, U)) for D, L, U in plain if MR.bwd_supported(D, L, U)}
    assert got == want and {n for *_, n in want} == {1, 4}
    refused = {(*MR.tiles(D, U), L) for D, L, U in plain if not MR.bwd_supported(D, L, U)}
    assert refused == {(*MR.tiles(D, U), L) for D, L, U in domain if D <= 32 and L <= 3 and not MR.bwd_supported(D, L, U)} != set()
    assert all(MR.backward_route(D, L, U, 1) == "wide" and MR.backward_route(D, L, U, 2) == "generic" for D, L, U in MR.wide_cases())
    assert {(MR.tiles(D, U), L) for D, L, U in MR.wide_cases()} == {((DT, UT), L) for DT in (3, 4) for UT in MR.UTS for L in (1, 2)}
    assert all(MR.backward_route(*g[:3], g[4]) == "generic" for g in MR.GENERIC_BWD)
    # backward, fused mode (NormFlow: U >= 15)
    fused = MR.train_cases()
    want = {(*MR.tiles(D, U), MR.nacc(D, L, U)) for D, L, U in domain if U >= 15 and MR.train_supported(D, L, U)}
    got = {(*MR.tiles(D, U), MR.nacc(D, L, U)) for D, L, U in fused if MR.train_supported(D, L, U)}
    assert got == want
    assert {(*MR.tiles(D, U), L) for D, L, U in fused} == {(DT, UT, L) for DT in (1, 2) for UT in MR.UTS for L in (1, 2, 3)}
    assert any(not MR.train_supported(*s) for s in fused)
    assert MR.bwd_supported(*MR.SMALL_WEIGHT[:3])


OLD_BARS = {"inverse": 2e-5, "sampling": 1e-4, "AR lp": 1e-5, "AR z0": 2e-5, "AR sld": 2e-5, "AR zf": 1e-4, "AR lq": 1e-4,
            "backward": 3e-5, "ar_train": 3e-5}


def test_noise_table(sweep):
    """The folded float32 noise of every group against the float64 oracle (and the float32 oracle's own, the generic
    kernels' bar): above 1e-9, and 4 x it inside the constant the suite has used for that quantity -- 2e-5 for inverse z
    and log-det (z0 and sum_log_det of the AR paths), 1e-4 * max(1, D // 8) >= 1e-4 for the sampling direction (the
    frozen forward's z and log_q), 1e-5 for log_prob, 3e-5 for gradients.  The small-weight case is its own group: its
    g_params noise is the absolute quantisation of r near 1/2 and is not held to the constant."""
    print("\n" + sweep.table())
    for (name, L), v in sorted(sweep.noise.items()):
        assert v > 1e-9, (name, L, v)
        if name.startswith("small-weight"):
            continue
        key = name.replace("generic ", "").replace("tile walk ", "").replace("unfused ", "")
        old = next(b for k, b in OLD_BARS.items() if key.startswith(k))
        assert 4.0 * v <= old, "%s L=%d: 4 x %.2e exceeds the suite's %.0e" % (name, L, v, old)
    small = sweep.noise[("small-weight backward g_params", 3)]
    assert small > 4.0 * sweep.noise[("backward g_params", 3)]  # the regime is a different one, hence a case of its own
