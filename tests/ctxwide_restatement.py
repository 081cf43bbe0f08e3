"""What the wide per-context tests share (tests/test_ctx_wide_host.py, tests/test_gpu_ctx_wide.py): the arithmetic of
csrc/flow_ctx_wide.hip and csrc/flow_ctx_wide_bwd.hip restated in torch (in the dtype of its inputs), their LDS formulas
and support predicates restated, and the GPU sweep's grid.  A helper like tests/wideflow_restatement.py: no test in here.

Inference.  The kernel walks the 2 S coupling layers ONE LAYER AT A TIME on two register halves of 16 HT slots (lo =
features 0 .. h-1, hi = features h .. D-1, zero above the real width): per layer it builds the layer's folded operand
image -- first-layer weights and biases scaled by c = 2 log2(e); hidden and output layers consuming r = (1 - tanh) / 2
with weights scaled by -2 c (hidden), -2 (t) and -2 log2(e) (s), the biases seeded with the weight's COLUMN SUM; `s` in
log2 units, so the coupling map is y 2^(+-s') -- and the fold block (A, B) of the BatchNorm / Affine maps, (1, 0) at a
padded slot.  That per-layer arithmetic is wideflow_restatement's (`folded_layer`, `fold_block`: csrc/wide_flow_tile.h is
shared by both kernels), and its `_walk` already visits one layer at a time, building each layer's image when it reaches
it; what differs here is the layout -- one parameter row per context, 1 <= N <= 31 -- so the two entries below call it with
M_p = M.  The padded slots stay inside what is restated: log_prob sums z0^2 over all 32 HT slots, as the kernel does.

Training.  The backward is the walk of csrc/ctx_bwd_walk.h on REAL widths (h, D - h and U: nothing is padded, no row
beyond N is formed): ctxtrain_restatement.log_prob_bwd with pad_to=None."""
import torch

import ctxtrain_restatement as T
import wideflow_restatement as W
from wideflow_restatement import coupling_params, flow_params, tiles  # noqa: F401 -- used by the tests

LDS_BUDGET = 150 * 1024  # kCtxWideLdsBudget
FWD, BWD = 0, 1  # `which` of tnf_ctx_wide_lds_bytes


# ---- the predicates ------------------------------------------------------------------------------------------------------
def in_domain(D, S, U, N):
    return 2 <= D <= 64 and S >= 1 and 17 <= U <= 64 and 1 <= N <= 31


def slice_floats(N, D, L, U):
    """ctx_bwd_slice_floats: zs, gs (N, D) | gl (N) | wb | act (2, L, N, U) | ts (2, N, D - h), rounded up to 4."""
    wb = max(coupling_params(D, L, U, True), coupling_params(D, L, U, False) + 2 * D)
    n = 2 * N * D + N + wb + 2 * L * N * U + 2 * N * (D - D // 2)
    return (n + 3) // 4 * 4


def lds_bytes(which, D, S, L, U, N):
    if not in_domain(D, S, U, N) or L < 1 or which not in (FWD, BWD):
        return -1
    return 4 * W.layer_floats(D, L, U) if which == FWD else 4 * slice_floats(N, D, L, U)


def ctx_wide_supported(D, S, L, U, N):
    return in_domain(D, S, U, N) and 1 <= L <= 5 and lds_bytes(FWD, D, S, L, U, N) <= LDS_BUDGET


def ctx_wide_train_supported(D, S, L, U, N):
    return in_domain(D, S, U, N) and 1 <= L <= 3 and lds_bytes(BWD, D, S, L, U, N) <= LDS_BUDGET


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def ctx_wide_log_prob(z, params, D, S, L, U, stat, defect=None):
    """tnf_ctx_wide_log_prob_f32 restated -> (log_prob, z0, sum_log_det).  z (M_z, N, D) with M_z in {1, M}, params (M, P)
    one row per context, stat = (mean (2S, D), alpha (2S, D)).  defect: None, "pad_weight" or "pad_fold"."""
    assert z.shape[1] <= 31 and z.shape[0] in (1, params.shape[0])
    return W.wide_flow_log_prob(z, params, D, S, L, U, stat, defect)


def ctx_wide_forward(omega, params, D, S, L, U, stat, defect=None):
    """tnf_ctx_wide_forward_f32 restated -> (z, sum_log_det, the largest |padded slot|)."""
    assert omega.shape[1] <= 31 and omega.shape[0] == params.shape[0]
    return W.wide_flow_forward(omega, params, D, S, L, U, stat, defect)


def ctx_wide_log_prob_bwd(z0, params, stat, g_lp, D, S, L, U):
    """tnf_ctx_wide_log_prob_bwd_f32 restated in float32 -> (g_params (M, P), g_z (M, N, D))."""
    return T.log_prob_bwd(z0, params, stat[0], stat[1], g_lp, D, S, L, U, pad_to=None)


# ---- the GPU sweep's grid ------------------------------------------------------------------------------------------------
DS = (4, 5, 32, 33, 64)
US = (17, 20, 32, 33, 48, 49, 64)
NS = (1, 15, 16, 17, 31)
MS = (1, 3, 5)
CDE_SHAPE = (4, 1, 2, 20)  # NormFlow(4, True, 'coupling', 1, 2, 20): the reference's own conditional-flow test, N = 1
S9_SHAPE = (5, 9, 2, 20)   # S is unbounded: beyond every image limit of the whole-flow wide kernel
L5_SHAPES = [(4, 1, 5, 20), (5, 2, 5, 33), (32, 1, 5, 64), (64, 1, 5, 48)]


def forward_shapes():
    """[(D, U)]: every D x U but each third one, which keeps every (HT, UT) cell and every D and U: 23 shapes."""
    out = [(D, U) for i, (D, U) in enumerate((D, U) for D in DS for U in US) if i % 3 != 2]
    assert {tiles(D, U) for D, U in out} == {(HT, UT) for HT in (1, 2) for UT in (2, 3, 4)}
    assert {D for D, _ in out} == set(DS) and {U for _, U in out} == set(US)
    return out


def forward_cases():
    """[(D, S, L, U, M, N)]: each shape of forward_shapes at L = 1, 2, 3 with S, M and N cycling through their lists; L = 5
    at four shapes; the reference's conditional-flow shape at N = 1; S = 9 at one small shape."""
    out, i = [], 0
    for D, U in forward_shapes():
        for L in (1, 2, 3):
            out.append((D, (1, 2)[i % 2], L, U, MS[i % 3], NS[i % 5]))
            i += 1
    for k, (D, S, L, U) in enumerate(L5_SHAPES):
        out.append((D, S, L, U, MS[k % 3], NS[(k + 1) % 5]))
    out.append(CDE_SHAPE + (5, 1))
    out.append(S9_SHAPE + (3, 17))
    assert all(ctx_wide_supported(D, S, L, U, N) for D, S, L, U, M, N in out)
    return out


def case_id(c):
    return "D%d-S%d-L%d-U%d-M%d-N%d" % tuple(c)
