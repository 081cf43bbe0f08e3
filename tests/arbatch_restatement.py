"""Sampling NormFlow('AR') = [MAF, BatchNorm, Affine] with fresh batch statistics (include/tnf_arbatch.h) restated in
torch, dtype-generic and without autograd: the forward by its definition, the backward by its closed form on top of
arsample_restatement.maf_sample_bwd.  tests/test_arbatch_host.py holds the backward to float64 autograd through
oracle.maf -> oracle.bn_forward_batch -> oracle.affine.

With n = M N rows in the batch, y = (z - b) e^-a the BatchNorm output,
    P_d = sum g_z e^a,   Q_d = sum g_z (z - b),   G = sum g_sld          (over ALL rows)
    g_x = g_z C0 + C1 + z C2,  C0 = e^a / alpha,  C2 = -e^-a (Q + G) / (n alpha),  C1 = -P / (n alpha) - b C2
    g_a = GZ - b GB + GS,  g_b = GB   with GZ = sum g_z z, GB = sum g_z, GS = sum g_sld per parameter row
and the MAF's share is maf_sample_bwd at (x = z A' + B', g_x, g_ld = g_sld), A' = alpha e^-a, B' = mean - b A'.

`folded=True` is the kernels' own formulation (csrc/ar_flow_batch.hip, maf_sample_bwd_body.h in its batch mode) on the
CPU: the sums in double from the float32 rows, the five coefficient rows formed in double and cast to float32, x and g_x
by float32 multiply-adds in the walk's load stage, the walk itself as arsample_restatement's folded float32 one.  In
float64 it is the same function; in float32 it is the noise model of the bars of tests/test_gpu_arbatch.py."""
import functools
import os
import sys

import numpy as np
import torch

import arsample_restatement as R
from maf_restatement import gerr

CAP = 2e-4  # tests/test_gpu_arsample.py: no gradient bar is looser than this
# (D, L, U, M, M_p, N) of tests/test_gpu_arbatch.py, forward and backward
TRAIN_SHAPES = [
    (6, 2, 15, 3, 3, 40),      # per-context rows, scalar accesses, a tail tile
    (5, 1, 20, 2, 1, 33),      # one shared row over two blocks of draws: the cross-context sums with M_p = 1
    (16, 2, 32, 2, 2, 50),     # float4 accesses, UT = 2
    (32, 3, 16, 1, 1, 40),     # DT = 2, L at its maximum
    (21, 2, 42, 2, 2, 100),    # the LFI shape: one shared accumulator copy
    (2, 1, 15, 1, 1, 2),       # n = 2 as one context of two rows
    (4, 2, 15, 2, 2, 1),       # n = 2 as two contexts of one row
    (8, 2, 15, 1, 1, 15), (8, 2, 15, 1, 1, 16), (8, 2, 15, 1, 1, 17),  # around one 16-row tile
    (4, 2, 15, 130, 130, 3), (4, 2, 15, 130, 1, 3),  # more contexts than a slice of the combine pass
    (4, 2, 15, 1, 1, 40000),   # several workgroups of pass 1 on one context, more tiles than a full grid's waves
]
FORWARD_ONLY = [(33, 1, 15, 2, 2, 40), (64, 2, 64, 1, 1, 40)]  # outside the backward's domain (D > 32)
LOSSES = (("both", 1.0, 1.0), ("z", 1.0, 0.0), ("log_q", 0.0, 1.0))
EPS = 1e-5  # BatchNorm's default


def shape_id(s):
    return "D%d_L%d_U%d_M%d_Mp%d_N%d" % s


def forward(oracle, omega, params, Ms, D, L, U, eps=EPS):
    """-> (z, sum_log_det, mean (D), alpha (D)) in the dtype of the inputs: statistics over all M N rows, biased variance."""
    n = oracle.maf_num_params(D, L, U)
    a, b = params[:, None, n:n + D], params[:, None, n + D:n + 2 * D]
    x, ld = oracle.maf(omega, params[:, :n], D, L, U, Ms, False)
    rows = x.reshape(-1, D)
    mean = rows.mean(0)
    alpha = torch.sqrt(((rows * rows).mean(0) - mean * mean).clamp_min(0.0) + eps)
    z = torch.exp(a) * ((x - mean) / alpha) + b
    return z, ld - torch.log(alpha).sum() + a.sum(2), mean, alpha


def backward(z, params, Ms, mean, alpha, g_z, g_sld, D, L, U, folded=False, drop_G=False, drop_P=False, context_n=False,
             drop_gs=False):
    """z (M, N, D) the stack's output, params (M_p, P_maf + 2 D), mean / alpha (D) the batch's statistics, cotangents
    g_z (M, N, D) and g_sld (M, N) -> g_params (M_p, P_maf + 2 D).  Four planted defects for tests/test_arbatch_host.py:
    `drop_G` leaves the log-det's cotangent out of C2, `drop_P` the mean's term out of C1, `context_n` divides by the
    rows of one context instead of the batch, `drop_gs` leaves GS out of g_a."""
    M, N = z.shape[:2]
    Mp = params.shape[0]
    n_maf = params.shape[1] - 2 * D
    wide = torch.float64 if folded else z.dtype  # the kernels keep the sums and form the coefficients in double
    a, b = params[:, n_maf:n_maf + D].to(wide), params[:, n_maf + D:].to(wide)
    zw, gw, sw = z.to(wide), g_z.to(wide), g_sld.to(wide)
    GZ, GB, GS = (gw * zw).sum(1), gw.sum(1), sw.sum(1)  # (M, D), (M, D), (M)
    P = (torch.exp(a) * GB).sum(0)
    Q = (GZ - b * GB).sum(0)
    G = 0.0 if drop_G else GS.sum()
    if drop_P:
        P = P * 0.0
    n = float(N if context_n else M * N)
    al, mu = alpha.to(wide), mean.to(wide)
    C0 = torch.exp(a) / al
    C2 = -torch.exp(-a) * (Q + G) / (n * al)
    C1 = -P / (n * al) - b * C2
    A = al * torch.exp(-a)
    B = mu - b * A
    A, B, C0, C1, C2 = (t.to(z.dtype)[:, None] for t in (A, B, C0, C1, C2))
    x = z * A + B
    g_x = g_z * C0 + (z * C2 + C1)
    g_maf = R.maf_sample_bwd(x, params[:, :n_maf], Ms, g_x, g_sld, D, L, U, folded=folded)[1]
    if Mp == 1:
        GZ, GB, GS = GZ.sum(0, keepdim=True), GB.sum(0, keepdim=True), GS.sum(0, keepdim=True)
    g_a = GZ - b * GB + (0.0 if drop_gs else 1.0) * GS[:, None]
    return torch.cat([g_maf, g_a.to(z.dtype), GB.to(z.dtype)], 1)


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import flow_oracle

    return flow_oracle


@functools.lru_cache(maxsize=None)
def problem(shape):
    """Inputs and float64 references of one shape, computed once and left unchanged: masks by the package's rule, MAF
    weights ~ N(0, 0.3), Affine ~ N(0, 0.2), omega and the loss weights ~ N(0, 1), all rounded to float32 first (the
    kernels' inputs).  z64 / sld64 / mean64 / alpha64: the float64 forward.  Per loss of LOSSES, loss = cz sum(z w_z) +
    cl sum(log_q w_l) with log_q = base - sum_log_det: `want[name]`, the float64 restatement at the float64 forward, and
    `noise[name]`, the error of the folded float32 restatement at the float32 rounding of that forward, over the whole
    parameter row (conftest.grad_err's measure, as tests/test_gpu_arsample.py takes it: relative to the largest entry of the
    gradient a training step applies); `noise_blocks[name]`: the same per block (MAF, Affine), for the record.  The two
    differ where one block's gradient all but vanishes: with n = 2 rows BatchNorm's output is +-1 / sqrt(1 + eps / var)
    whatever x is, so d z / d x is of order eps and the MAF block of the z-only loss is 1e-5 of the Affine slice -- rebuilt
    from a float32 z it carries 1e-2 of its own size in any float32 route, 1e-7 of the row."""
    import torch_nf_amd as tnf

    oracle = _oracle()
    D, L, U, M, Mp, N = shape
    rng = np.random.RandomState(1000 * D + 10 * L + U + M + N)
    np.random.seed(D + L)
    maf = tnf.MAF(D, L, U)
    ms = [np.array(m) for m in maf.ms]
    Ms = [Mk[0].numpy().astype(np.float64) for Mk in maf.Ms]
    n = maf.count_num_params()
    f32 = lambda t: torch.tensor(t).float()  # noqa: E731
    pr = dict(ms=ms, Ms=Ms, n=n,
              params=torch.cat([f32(rng.normal(0, 0.3, (Mp, n))), f32(rng.normal(0, 0.2, (Mp, 2 * D)))], 1),
              omega=f32(rng.normal(0, 1, (M, N, D))), wz=f32(rng.normal(0, 1, (M, N, D))), wl=f32(rng.normal(0, 1, (M, N))))
    with torch.no_grad():
        z, sld, mean, alpha = forward(oracle, pr["omega"].double(), pr["params"].double(), Ms, D, L, U)
        pr.update(z64=z, sld64=sld, mean64=mean, alpha64=alpha)
        if D <= 32:
            pr["want"], pr["noise"], pr["noise_blocks"] = {}, {}, {}
            z32, stat32 = z.float(), (mean.float(), alpha.float())
            for name, cz, cl in LOSSES:
                g_z, g_sld = cz * pr["wz"], -cl * pr["wl"]  # d loss / d sum_log_det = -cl w_l
                pr["want"][name] = backward(z, pr["params"].double(), Ms, mean, alpha, g_z.double(), g_sld.double(), D, L, U)
                fold = backward(z32, pr["params"], Ms, *stat32, g_z, g_sld, D, L, U, folded=True)
                pr["noise"][name] = gerr(fold, pr["want"][name])
                pr["noise_blocks"][name] = split_err(fold, pr["want"][name], n)
    return pr


def split_err(got, want, n):
    """(MAF block, Affine slice): max |got - want| / max |want| of each."""
    return gerr(got[:, :n], want[:, :n]), gerr(got[:, n:], want[:, n:])
