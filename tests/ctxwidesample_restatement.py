"""The cases of the backward of frozen-statistics sampling above 16 units (include/tnf_ctxwidesample.h,
csrc/flow_ctx_wide_sample_bwd.hip), shared by tests/test_ctx_wide_sample_host.py (the restatement alone, on the CPU) and
tests/test_gpu_ctx_wide_sample.py (the kernel).  The walk is that of csrc/flow_ctx_sample_bwd.hip, whose float32
restatement (tests/ctxsample_restatement.py) is width-agnostic: `sample_bwd`, `reference`, `upstream` and `row_err` are
its.  A case is (D, S, L, U, M, N): the smallest shapes at which each mechanism can go wrong."""
import collections

import ctxwide_restatement as W
from ctxsample_restatement import reference, row_err, sample_bwd, upstream  # noqa: F401  (re-exported)

WIDTHS, SAMPLES = (2, 5, 16, 31, 32, 33, 63, 64), (1, 2, 15, 16, 17, 31)
TEAM_SIZES = (4, 8, 16)
# one sample at the reference's conditional-flow shape; one context, one sample at the widest layer; 49 units with two
# tiles of samples; the largest slice at L <= 2 (123,008 B); a large one at L = 3 (144,512 B); the last N that fits at
# D = 64, L = 3, U = 64
TEAMS_AND_SLICES = [(4, 1, 2, 20, 5, 1), (64, 1, 2, 64, 1, 1), (32, 1, 1, 49, 2, 17), (64, 1, 2, 64, 2, 31),
                    (33, 1, 3, 64, 2, 31), (64, 1, 3, 64, 2, 22)]
ONE_COTANGENT = [(5, 2, 2, 20, 5, 17), (64, 1, 3, 48, 3, 31)]


def groups():
    """{group: [(D, S, L, U, M, N)]}: the cases, in the groups that share a bar."""
    out = collections.OrderedDict()
    out["widths_and_samples"] = [(D, 2, 2, 20, 5, N) for D in WIDTHS for N in SAMPLES]
    for S in (1, 9):
        for L in (1, 3):
            out["depth_and_units S=%d L=%d" % (S, L)] = [(D, S, L, U, 3, 7) for D in (5, 64) for U in (17, 48, 64)]
    out["teams_and_slices"] = list(TEAMS_AND_SLICES)
    return out


def group_of(case):
    for name, cases in groups().items():
        if case in cases:
            return name
    raise KeyError(case)


GRID = [c for cases in groups().values() for c in cases]


def case_id(c):
    return "D%d-S%d-L%d-U%d-M%d-N%d" % tuple(c)


def sample_supported(D, S, L, U, N):
    """tnf_ctx_wide_sample_supported restated: the forward's predicate and the backward's, both."""
    return W.ctx_wide_supported(D, S, L, U, N) and W.ctx_wide_train_supported(D, S, L, U, N)


def auto_waves(D, U, N):
    """tnf_ctx_wide_sample_waves restated: the shipped team-size rule, -1 outside the domain."""
    if not W.in_domain(D, 1, U, N):
        return -1
    if (N <= 8 and 2 * U * U <= 1024) or (N == 1 and U > 48 and D <= 8):  # the two measured departures from the log_prob direction's rule
        return 4
    if N > 16 and U > 48 and D >= 32:
        return 16
    widest = 2 * U * max(U, (D + 1) // 2)
    return 4 if widest <= 1024 else 8


def group_bar(bar, restatement):
    """The group's bar: the suite's, unless the float32 restatement alone exceeds a quarter of it -- then 4 x its error
    (the rule of tests/test_gpu_ctx_wide.py)."""
    return bar if restatement <= bar / 4 else 4.0 * restatement


# ---- the restatement's own error, and the bars that follow from it ---------------------------------------------------------
def forward32(oracle, omega, params, mean, alpha, shape):
    """The float32 z the kernel starts from: the oracle's frozen-statistics sampling pass in float32."""
    import torch

    with torch.no_grad():
        return oracle.flow_forward(omega.double().numpy(), params, *shape, bn_stats=list(zip(mean, alpha)))[0]


_ERRS, _BARS = {}, {}


def restatement_errors(oracle, case):
    """{"params", "omega"}: the float32 restatement of the walk from a float32 z against float64 autograd, the larger of
    the whole and the per-row error; computed once per case."""
    if case not in _ERRS:
        from conftest import grad_err
        from domain_helpers import float64
        from test_gpu_ctx_flow import inputs

        D, S, L, U, M, N = case
        params, mean, alpha, omega = inputs(oracle, *case)
        g_z, g_sld = upstream(M, N, D)
        shape = (D, S, L, U)
        z = forward32(oracle, omega, params, mean, alpha, shape)
        gp, go, _ = sample_bwd(z, params, mean, alpha, g_z, g_sld, *shape)
        want = reference(oracle, float64, omega, params, mean, alpha, g_z, g_sld, shape, key=case)
        _ERRS[case] = {"params": max(grad_err("ctxwidesample restatement params", gp, want[0]), row_err(gp, want[0])),
                       "omega": max(grad_err("ctxwidesample restatement omega", go, want[1]), row_err(go, want[1]))}
    return _ERRS[case]


def bars(oracle, group):
    """(bar for the parameters, bar for omega) of a group: BAR_P and BAR_Z under `group_bar`, from the restatement on the
    group's own cases, on the host the test runs on.  The kernel never enters its own bar."""
    if group not in _BARS:
        from domain_helpers import BAR_P, BAR_Z

        errs = [restatement_errors(oracle, c) for c in groups()[group]]
        _BARS[group] = (group_bar(BAR_P, max(e["params"] for e in errs)), group_bar(BAR_Z, max(e["omega"] for e in errs)))
    return _BARS[group]
