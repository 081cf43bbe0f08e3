"""What the domain sweeps share (tests/test_gpu_domain.py, tests/test_gpu_cond_domain.py,
tests/test_gpu_support_domain.py): the float64 context of the oracle, the kernel-variant switch, the launch counters, the
conditional-estimator input scheme and the suite's existing bars.  A helper like tests/mog_restatement.py: no test in
here."""
import contextlib
import copy

import torch

from torch_nf_amd import _lib as L_

lib = L_.lib

LOGP_TOL = dict(rtol=1e-5, atol=1e-5)   # LOGP_RTOL of test_gpu_parity.py
INV_TOL = dict(rtol=1e-4, atol=1e-4)    # z0 and sum_log_det: test_full_size_properties
ZF_TOL = dict(rtol=2e-5, atol=1e-5)     # z of the sampling direction: test_oracle_forward_many_contexts
LQ_TOL = dict(rtol=1e-5, atol=2e-5)     # log_q: test_oracle_forward_many_contexts
SLDF_TOL = dict(rtol=1e-4, atol=1e-4)   # forward sum_log_det: test_full_size_properties
BAR_P, BAR_Z = 5e-5, 5e-6               # test_flow_level_training_pair (4 x the measured reversible-pair errors)

FORWARD_FAMILIES = (L_.DIAG_FLOW_FUSED2, L_.DIAG_FLOW_FUSED2_FWD, L_.DIAG_FLOW_FUSED3, L_.DIAG_FLOW_F16, L_.DIAG_FLOW_FP32,
                    L_.DIAG_FLOW_RANGE2, L_.DIAG_FLOW_RANGE2_FWD, L_.DIAG_COUPLING_MFMA)


@contextlib.contextmanager
def float64():
    """Run the oracle in double precision: its intermediate buffers follow torch's default dtype."""
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(before)


@contextlib.contextmanager
def variants(flow=10, layer=10):
    """Select the whole-flow and per-layer kernel variants for the block; the defaults (10, 10) come back afterwards."""
    L_.check(lib.tnf_set_option(L_.OPT_FLOW_VARIANT, flow))
    L_.check(lib.tnf_set_option(L_.OPT_LAYER_VARIANT, layer))
    try:
        yield
    finally:
        L_.check(lib.tnf_set_option(L_.OPT_FLOW_VARIANT, 10))
        L_.check(lib.tnf_set_option(L_.OPT_LAYER_VARIANT, 10))


def counts():
    torch.cuda.synchronize()
    return [lib.tnf_diag_launch_count(f) for f in range(L_.DIAG_FAMILIES)]


def launched(before, families=None):
    """{family: launches since `before`} (only the families that moved, restricted to `families` when given)."""
    after = counts()
    return {f: a - b for f, (a, b) in enumerate(zip(after, before)) if a != b and (families is None or f in families)}


def _cde(tnf, D, S, L, H, seed, Dx=8, U=15):
    torch.manual_seed(seed)
    nf = tnf.NormFlow(D, True, "coupling", S, L, U)
    cde = tnf.ConditionalDensityEstimator(nf, Dx, [H])
    g = torch.Generator().manual_seed(seed)
    for b in nf._bn_layers():
        b.set_last_stats(torch.randn(D, generator=g) * 0.1, torch.rand(D, generator=g) * 0.5 + 0.75)
    with torch.no_grad():
        for p in cde.param_net.parameters():
            p.mul_(0.5)
    cde.cuda()
    return nf, cde


def _net64(cde):
    return copy.deepcopy(cde.param_net).cpu().double()


def _stats64_of(nf):
    return [(b.get_last_mean().cpu().double(), b.get_last_alpha().cpu().double()) for b in nf._bn_layers()]
