"""NormFlow with the reference's interface, executing on MI355X.

Drop-in for DensityEstimator / NormFlow of the reference's
torch_nf/density_estimator.py (:11-55, :240-421): same constructor, validation,
bijector stack, flat-parameter slicing, `__call__(N, params, freeze_bn)`,
`forward`, `inverse_and_log_det`, `log_prob`, `count_num_params`, `D_params`,
`params`, `bijectors`.

Execution: `NormFlow._route` names the kernel family of every call; each public operation stages its inputs, asks it
once and runs that one arm.  First match wins, top to bottom.  "plain" = z and params float32 and, with grad mode on,
neither requires grad; "const stats" = the cached BatchNorm statistics carry no graph (`_stats_in_graph()` is False:
only the per-bijector composition differentiates through them); "not few" = not (several parameter rows and fewer than
32 samples each); "3-d" = z is (M, N, D).  The entries that take (z, params, statistics, shape) and nothing else are
reached through one lookup per operation (`_SAMPLERS`, `_DENSITIES`, `_TRAINERS`: family -> module, attribute) where
they belong to the seven one-launch coupling families; the per-context families up to 16 units and their `_wide` twins
share a predicate each, asked twice (`_PER_CONTEXT`: switch -> `*_supported` function, measured exclusion).

  family            offered to           conditions                                                  ops entry
  ----------------  -------------------  ----------------------------------------------------------  --------------------
  batch_chain       forward, fresh       fused's conditions, fused_batch_forward, one parameter row  flow_forward_batch_raw
                    statistics           per z row, flow_train_supported at N = 32, and M*N > 1 or
                                         batch_stats_reduce set
  batch_train       forward, fresh       coupling, float32, batch_stats_reduce unset, the chain's    flow_forward_train
                    statistics           shape conditions, M*N >= 32 (one autograd node)
  batch_chain_      forward, fresh       padded_batch_forward (default off), coupling, inference,    padbatch_ops.flow_padded_
  padded            statistics           3-d, one parameter row per z row, batch_stats_reduce unset, forward_batch_raw
                                         fusion AUTO or FLOW, flow_padded_batch_supported (2 <= D <=
                                         63 but 32: widths the two above never take), M*N > 1
  batch_train_      forward, fresh       the same with float32 in place of inference, M*N >= 32      padbatch_ops.flow_padded_
  padded            statistics           (one autograd node)                                         forward_train
  ar_fused          forward (frozen),    AR, plain, const stats, 3-d, ar_flow_supported; forward:    ar_flow_forward_raw,
                    log_prob, inverse    support layer absent or ToInterval                          ar_flow_log_prob_raw
  ar_train          log_prob             AR, fused_ar_training, grad mode on, const stats, float32,  ar_flow_log_prob_train
                                         params requires grad and z does not, 3-d, M_z >= M_p,
                                         ar_flow_supported, ar_flow_train_supported
  ar_train_sample   forward (frozen)     ar_sample_training (default off), AR, float32, grad mode    arsample_ops.ar_flow_
                                         on and params requires grad, const stats, 3-d, M_p = 1 or   sample_train
                                         M_z, any support layer (run behind it as its own op),
                                         ar_flow_supported, maf_sample_bwd_supported, operand
                                         precision 0 (asked after ar_fused, which takes the calls
                                         without a gradient)
  ar_batch_chain    forward, fresh       ar_batch_forward (default off), AR, plain, 3-d, one         arbatch_ops.ar_flow_
                    statistics           parameter row per z row, M*N >= 2, batch_stats_reduce       forward_batch_raw
                                         unset, M*N*D <= 160,000 (a tie above: DESIGN.md 22),
                                         ar_flow_batch_supported; any support layer runs behind it
                                         as its own op
  ar_batch_train    forward, fresh       the same at any batch size with float32 in place of plain,  arbatch_ops.ar_flow_
                    statistics           grad mode on and params requires grad, operand precision    forward_batch_train
                                         0, ar_flow_batch_train_supported (D <= 32; one autograd
                                         node)
  padded            forward (frozen),    coupling, plain, const stats, not few, 3-d, fusion AUTO or  flow_padded_forward_raw,
                    log_prob, inverse    FLOW, flow_padded_supported                                 flow_padded_log_prob_raw
  wide_flow         forward (frozen),    wide_flow (default off), coupling, plain, const stats, not  wideflow_ops.wide_flow_
                    log_prob, inverse    few, 3-d, fusion AUTO or FLOW, wide_flow_supported (17 <=   forward_raw, wide_flow_
                                         num_units <= 64, any 2 <= D <= 64, the 2 S operand images   log_prob_raw
                                         within the LDS budget), and not (forward with several
                                         parameter rows at D % 8 == 0, D < 32: the wide chain is
                                         faster there) (asked before fused: with the
                                         switch on it takes the D % 8 == 0 shapes from the wide
                                         per-layer chain)
  wide_flow_        forward (frozen),    wide_flow_streamed (default off); wide_flow's conditions    widestream_ops.wide_flow_
  streamed          log_prob, inverse    with wide_flow_supported 0 and wide_flow_stream_supported   stream_forward_raw, wide_
                                         1 (17 <= num_units <= 64, any 2 <= D <= 64, ONE layer's     flow_stream_log_prob_raw
                                         operand image within the LDS budget, 1 <= S <= 1024: the
                                         stage counts the resident kernel cannot hold), and not
                                         (D % 8 == 0 unless z and params are one row each with
                                         N <= 2^17, forward: N <= 2^12: the wide per-layer chain
                                         is faster or ties beyond)
                                         (wide_flow's own sampling exclusion is not copied; asked
                                         right after wide_flow: the shape sets are disjoint
                                         whatever the switches say)
  fused             forward (frozen),    coupling, plain, const stats, not few, has_fast_path        flow_forward_raw,
                    log_prob, inverse    (`_fused_ok`; whole flow or per-layer chain as `fusion`     flow_log_prob_raw
                                         resolves)
  train_reversible  log_prob             coupling, float32, const stats, 3-d, M_z >= M_p,            flow_log_prob_train
                                         reversible_training, flow_train_rev_supported               (reversible=True)
  train_layers      log_prob             the same, flow_train_supported                              (reversible=False)
  train_padded      log_prob             padded_training (default off), coupling, float32, const     padtrain_ops.flow_padded_
                                         stats, 3-d, M_z >= M_p, one parameter row or 32 samples     log_prob_train
                                         per row, fusion AUTO or FLOW, flow_padded_train_supported
                                         (2 <= D <= 63 but 32: asked after train_reversible, whose
                                         widths it excludes, and before train_layers)
  train_context     log_prob             context_training (default off), coupling, float32, grad     ctxtrain_ops.ctx_flow_
                                         mode on and params or z requires grad, const stats, 3-d,    log_prob_train
                                         several parameter rows = the larger batch, M_z = M (or 1
                                         when z does not require grad), 1 <= N <= 31, fusion AUTO or
                                         FLOW, ctx_train_supported (asked after the training pairs
                                         above: only calls that would otherwise compose bijectors)
  train_context_    log_prob             wide_context_training (default off); train_context's        ctxwide_ops.ctx_wide_
  wide                                   conditions with ctx_wide_train_supported (17 <= num_units   log_prob_train
                                         <= 64, num_layers <= 3, the context's backward slice within
                                         150 KB of LDS) in place of ctx_train_supported (asked right
                                         after train_context: the unit ranges are disjoint)
  train_sample      forward (frozen)     sample_training (default off), coupling, float32, grad      sampletrain_ops.flow_
                                         mode on and params requires grad, const stats, 3-d, one     sample_train
                                         parameter row or 32 samples per row, fusion AUTO or FLOW,
                                         flow_sample_train_supported (asked after padded and fused,
                                         which take the calls without a gradient)
  train_context_    forward (frozen)     context_sample_training (default off), coupling, float32,   ctxsample_ops.ctx_flow_
  sample                                 grad mode on and params requires grad, const stats, 3-d,    sample_train
                                         several parameter rows, one block of draws per row,
                                         1 <= N <= 31, fusion AUTO or FLOW, ctx_sample_supported
                                         (asked after train_sample, which takes one parameter row
                                         or 32 samples per row; independent of context_rows and
                                         context_training)
  train_context_    forward (frozen)     wide_context_sample_training (default off);                 ctxwidesample_ops.ctx_
  sample_wide                            train_context_sample's conditions with                      wide_sample_train
                                         ctx_wide_sample_supported (17 <= num_units <= 64,
                                         num_layers <= 3, one layer's operand image and the
                                         context's backward slice within 150 KB of LDS) in place of
                                         ctx_sample_supported (asked right after
                                         train_context_sample: the unit ranges are disjoint;
                                         independent of every other switch)
  context_rows      forward (frozen),    context_rows (default off), coupling, plain, const stats,   ctxflow_ops.ctx_flow_
                    log_prob, inverse    3-d, several parameter rows = the larger batch, M_z = 1 or  forward_raw, ctx_flow_
                                         M (forward: M), 1 <= N <= 31, fusion AUTO or FLOW,          log_prob_raw
                                         ctx_flow_supported, and not (log_prob or inverse at D = 64
                                         with N <= 5: the per-layer composition is faster there,
                                         DESIGN.md 18) (asked last: only calls that would otherwise
                                         compose bijectors)
  context_rows_     forward (frozen),    wide_context_rows (default off); context_rows' conditions   ctxwide_ops.ctx_wide_
  wide              log_prob, inverse    with ctx_wide_supported (17 <= num_units <= 64, num_layers  forward_raw, ctx_wide_
                                         <= 5, one layer's operand image within 150 KB of LDS) in    log_prob_raw
                                         place of ctx_flow_supported and without the D = 64
                                         exception, and not (N = 1 with num_units > 48: the
                                         composition is faster there) (asked right
                                         after context_rows: the unit ranges are disjoint)
  bijectors         all                  everything else: the reference's loop, one kernel per       coupling, maf, affine,
                                         bijector                                                    bn_apply, bn_batch_forward

Support layer (ToInterval / ToSimplex, the last bijector).  ar_fused, ar_train and the whole-flow `fused` kernel evaluate
a ToInterval layer in their own load / store stage (`Route.fuse_support`); `padded`, `train_padded`, `train_context`,
`context_rows`, `context_rows_wide`, `train_context_wide`, `wide_flow`, `wide_flow_streamed`, `train_sample`, `train_context_sample`, `train_context_sample_wide`, `ar_train_sample`, the batch-statistics chains (padded or not) and
the per-layer chain do not.
Otherwise it is one extra elementwise kernel: after the stack in `forward`, before the core route in `log_prob`.
`inverse_and_log_det` of a flow with a support layer is always `bijectors` over the whole stack.
Sampling: the base density is evaluated first (base_log_density_f64), except that `padded`, the whole-flow `fused`
kernel and `train_sample` (whose forward is one of those two) write log_q themselves for a float32 tensor draw
(`Route.writes_log_q`).
"""
import collections

import numpy as np
import torch

from . import (_lib, arbatch_ops, arsample_ops, ctxflow_ops, ctxsample_ops, ctxtrain_ops, ctxwide_ops, ctxwidesample_ops, ops,
               padbatch_ops, padtrain_ops, sampletrain_ops, wideflow_ops, widestream_ops)
from .bijectors import MAF, Affine, BatchNorm, Bijector, RealNVP, _Checked


# a call's route: the kernel family, whether that kernel evaluates the support layer itself, and (sampling) whether it
# writes log_q itself
Route = collections.namedtuple("Route", "family fuse_support writes_log_q")
_BIJECTORS, _FUSED = Route("bijectors", False, False), Route("fused", False, False)  # the two commonest, built once

# The arms of the seven one-launch coupling families, which all take (z, params, *NormFlow._flow_args()) and nothing else,
# per operation: family -> (module, attribute), resolved with getattr when the call is made (the host tests replace
# `module.attribute` by recorders).
# None of them evaluates a support layer: it runs as its own kernel.
_SAMPLERS = {  # NormFlow._forward_from, frozen statistics -> (z, sum_log_det)
    "context_rows": (ctxflow_ops, "ctx_flow_forward_raw"),  # one wave per context
    "context_rows_wide": (ctxwide_ops, "ctx_wide_forward_raw"),  # one workgroup per context
    "wide_flow": (wideflow_ops, "wide_flow_forward_raw"),  # one workgroup per parameter row
    "wide_flow_streamed": (widestream_ops, "wide_flow_stream_forward_raw"),  # ... the layers' images streamed through LDS
    "train_context_sample": (ctxsample_ops, "ctx_flow_sample_train"),  # one autograd node, one launch each way
    "train_context_sample_wide": (ctxwidesample_ops, "ctx_wide_sample_train"),  # ... above 16 units
}
_DENSITIES = {  # NormFlow._fused_density (want_lp, want_z0, want_sld) -> (log_prob | None, z0 | None, sum_log_det | None)
    "context_rows": (ctxflow_ops, "ctx_flow_log_prob_raw"),
    "context_rows_wide": (ctxwide_ops, "ctx_wide_log_prob_raw"),
    "wide_flow": (wideflow_ops, "wide_flow_log_prob_raw"),
    "wide_flow_streamed": (widestream_ops, "wide_flow_stream_log_prob_raw"),
}
_TRAINERS = {  # NormFlow.log_prob under autograd, the BatchNorm statistics constant -> log_prob
    "train_context": (ctxtrain_ops, "ctx_flow_log_prob_train"),  # per-context rows, fewer than 32 samples each
    "train_context_wide": (ctxwide_ops, "ctx_wide_log_prob_train"),  # ... at 17 <= num_units <= 64
}


def _context_rows_slower(op, shape, N):
    """The measured exclusion of `context_rows` (profiles/r14_ctxbench.txt): the inverse direction at
    D = 64 with at most 5 samples per context stays on the composition, whose fp32-MFMA layer kernel is faster there
    (0.82 x at N = 1 .. 0.97 x at N = 4; 1.07 x at N = 6)."""
    return op != "forward" and shape[0] == 64 and N <= 5


def _context_rows_wide_slower(op, shape, N):
    """The measured exclusion of `context_rows_wide` (profiles/r22_ctxwidebench.txt; M N = 2^16, S = 2,
    L = 2): ONE sample per context above 48 units, every op, where a workgroup builds every layer's 70 .. 134 KB image
    for a single row of z and the composition's per-layer kernels stream the same parameters faster (0.89 .. 0.98 x at
    num_units = 64, D = 4 .. 64; 1.27 .. 1.59 x at N = 8).  The C entries accept the class all the same.  The D = 64,
    N <= 5 exception of `context_rows` is a measurement of the 16-unit kernel and is not copied."""
    return N == 1 and shape[3] > 48


# What `NormFlow._route` asks each per-context predicate with, twice: switch -> (module, its `*_supported` function by
# name, the family's measured exclusion or None).  Read only once the switch has tested true, with getattr at that time:
# with a switch off, the call costs that one test.
_PER_CONTEXT = {
    "context_rows": (ctxflow_ops, "ctx_flow_supported", _context_rows_slower),
    "wide_context_rows": (ctxwide_ops, "ctx_wide_supported", _context_rows_wide_slower),
    "context_training": (ctxtrain_ops, "ctx_train_supported", None),
    "wide_context_training": (ctxwide_ops, "ctx_wide_train_supported", None),
    "context_sample_training": (ctxsample_ops, "ctx_sample_supported", None),
    "wide_context_sample_training": (ctxwidesample_ops, "ctx_wide_sample_supported", None),
}


def _min_two(val):
    if val < 2:
        raise ValueError("DensityEstimator D %d must be greater than 1." % val)
    return val


class DensityEstimator(object):
    """Abstract base (density_estimator.py:11-55)."""

    D = _Checked("D", int, _min_two)
    conditioner = _Checked("conditioner", bool)

    def __init__(self, D, conditioner=False):
        super().__init__()
        self.D = D
        self.conditioner = conditioner

    def __call__(self, N=100, params=None):
        if not self.conditioner:
            return self.forward(self.params, N)
        return self.forward(params, N)

    def forward(self, params, N=100, freeze_bn=False):
        raise NotImplementedError()

    def log_prob(self, z, params=None):
        raise NotImplementedError()

    def count_num_params(self):
        raise NotImplementedError()

    def _param_init(self):
        raise NotImplementedError()


def _arch(val):
    if val not in ("coupling", "AR", "affine"):
        raise ValueError('NormalizingFlow arch_type must be "coupling", "AR", or "affine".')
    return val


def _stages(val):
    if val < 1:
        raise ValueError("NormalizingFlow num_stages %d must be greater than 0." % val)
    return val


def _layers(val):
    if val < 1:
        raise ValueError("NormalizingFlow num_layers arg %d must be greater than 0." % val)
    return val


def _units(val):
    if val < 1:
        raise ValueError("NormalizingFlow num_units %d must be greater than 0." % val)
    if val < 15:
        print("Warning: NormFlow.num_layers set to minimum of 15 (received %d)." % val)
        return 15
    return val


class NormFlow(DensityEstimator):
    """Normalizing flow q(z) = N(omega; 0, I) pushed through a bijector stack
    (density_estimator.py:240-421).

    arch_type="coupling": num_stages x [RealNVP(upper), BatchNorm, RealNVP(lower),
    BatchNorm, Affine] (:260-270).  All bijector parameters live in one flat row
    `params` (1, D_params) -- or are supplied per context as (M, D_params) when
    conditioner=True -- and are consumed front-to-back by `forward` (:379-384) and
    back-to-front by `inverse_and_log_det` (:399-402).

    Extra (not in the reference): `device` -- where the flow's own `params` live
    (default: the current HIP device when there is one).
    """

    arch_type = _Checked("arch_type", str, _arch)
    num_stages = _Checked("num_stages", int, _stages)
    num_layers = _Checked("num_layers", int, _layers)
    num_units = _Checked("num_units", int, _units)
    # frozen-statistics sampling under autograd through one backward kernel (family `train_sample`); off: today's route
    sample_training = False
    # the same for arch_type "AR" (family `ar_train_sample`); with fresh statistics the per-bijector composition runs
    # with the MAF's one-kernel sampling backward (MAF.fused_sampling_backward) for the call; off: today's routes
    ar_sample_training = False
    # fresh-statistics sampling of arch_type "AR" -- nf(N), cde(x, N) -- as one C call forward and one backward (families
    # `ar_batch_chain` / `ar_batch_train`); off: today's per-bijector composition
    ar_batch_forward = False
    # frozen-statistics sampling under autograd with several parameter rows and fewer than 32 draws per row -- cde(x, N,
    # freeze_bn=True) with a handful of draws per x -- through one backward launch (family `train_context_sample`); off:
    # today's per-bijector composition
    context_sample_training = False
    # plain log_prob, inverse_and_log_det, frozen forward and sample with 17 <= num_units <= 64 as one launch at any
    # 2 <= D <= 64 (family `wide_flow`, csrc/flow_wide.hip); off: today's wide per-layer chain or per-bijector composition
    wide_flow = False
    # the same calls at the stage counts that kernel cannot hold in LDS -- S > 4, 2, 1 or 0 by shape -- as one launch with
    # the layers' operand images streamed through LDS (family `wide_flow_streamed`, csrc/flow_wide_stream.hip); off:
    # today's wide per-layer chain or per-bijector composition.  Independent of `wide_flow`: the shape sets are disjoint
    wide_flow_streamed = False
    # plain log_prob, inverse_and_log_det, frozen forward and sample with 17 <= num_units <= 64, several parameter rows
    # and fewer than 32 samples per row as one launch (family `context_rows_wide`, csrc/flow_ctx_wide.hip); off: today's
    # per-bijector composition
    wide_context_rows = False
    # the same layout's log_prob under autograd as one launch each way (family `train_context_wide`,
    # csrc/flow_ctx_wide_bwd.hip); off: today's per-bijector composition.  Independent of `wide_context_rows`
    wide_context_training = False
    # the same layout's frozen-statistics sampling under autograd -- cde(x, N, freeze_bn=True) with a handful of draws per
    # x, then loss(z, log_q).backward() -- as one launch each way (family `train_context_sample_wide`,
    # csrc/flow_ctx_wide_sample_bwd.hip); off: today's per-bijector composition.  Independent of every other switch
    wide_context_sample_training = False

    def __init__(self, D, conditioner=False, arch_type="AR", num_stages=1, num_layers=2,
                 num_units=15, support_layer=None, device=None):
        super().__init__(D, conditioner)
        self.arch_type = arch_type
        self.num_stages = num_stages
        self.num_layers = num_layers
        self.num_units = num_units
        self.support_layer = support_layer
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
                else torch.device("cpu")
        self.device = torch.device(device)
        self.fusion = _lib.FUSE_AUTO
        # sample-sharded sampling with fresh statistics (one process per GPU): a callable that sums a BatchNorm layer's
        # [sum | sum of squares | count] moments over the ranks sharing the batch (distributed.moment_reducer(group))
        self.batch_stats_reduce = None

        self.bijectors = []
        if self.arch_type == "coupling":
            for _ in range(self.num_stages):
                self.bijectors.append(RealNVP(D, self.num_layers, self.num_units, transform_upper=True))
                self.bijectors.append(BatchNorm(D))
                self.bijectors.append(RealNVP(D, self.num_layers, self.num_units, transform_upper=False))
                self.bijectors.append(BatchNorm(D))
                self.bijectors.append(Affine(D))
        elif self.arch_type == "AR":  # density_estimator.py:271-274
            self.bijectors.append(MAF(D, self.num_layers, self.num_units, fwd_fac=True))
            self.bijectors.append(BatchNorm(D))
            self.bijectors.append(Affine(D))
        else:
            self.bijectors.append(Affine(D))

        self._n_core = len(self.bijectors)  # the parameterised stack; a support layer comes after it
        if support_layer is not None:
            if issubclass(type(support_layer), Bijector):
                self.bijectors.append(support_layer)  # density_estimator.py:278-282
            else:
                raise TypeError("Support layer not Bijector.")

        self.count_num_params()
        if not self.conditioner:
            self._param_init()

    # -- parameters ---------------------------------------------------------
    def count_num_params(self):
        """density_estimator.py:418-421."""
        self.D_params = 0
        for bijector in self.bijectors:
            self.D_params += bijector.count_num_params()

    def _param_init(self):
        """xavier_normal_ on a (1, D_params) row (density_estimator.py:352-356); drawn on the
        host so torch.manual_seed reproduces the reference's initialisation, then moved."""
        init = torch.nn.init.xavier_normal_(torch.zeros(1, self.D_params))
        self.params = init.to(self.device).requires_grad_(True)
        return None

    # -- helpers ------------------------------------------------------------
    def _bn_layers(self):
        return [b for b in self.bijectors if b.name == "BatchNorm"]

    def _bn_stats(self, dev):
        """(2S, D) stacks of the cached BatchNorm statistics on `dev`; rebuilt only when a
        BatchNorm layer's statistics changed (keeps the per-call host work off the hot path)."""
        bns = self._bn_layers()
        key = (dev, tuple(b._version for b in bns))
        cached = self.__dict__.get("_bn_cache")
        if cached is None or cached[0] != key:
            mean = torch.stack([b.get_last_mean().detach().float().to(dev) for b in bns])
            alpha = torch.stack([b.get_last_alpha().detach().float().to(dev) for b in bns])
            cached = (key, mean, alpha)
            self.__dict__["_bn_cache"] = cached
        return cached[1], cached[2]

    def _facts(self, z, params):
        """What several families ask of a call, computed once, as the plain tuple (arch_type, (D, S, L, U),
        stats_graph, f32, plain, inference): the configuration (every read of it runs a validating descriptor); the
        statistics carry a graph; z and params are float32; the call is plain (float32 and nothing requires grad); it
        is inference for the one-call coupling kernels (a coupling stack, plain, constant statistics, and not
        per-context weights with fewer than 32 samples each -- the SNPE layout, N = 1, whose prepared operand images,
        ~100 KB per context, would outweigh the samples).  A tuple, not a class: this runs on every call."""
        arch, grad = self.arch_type, torch.is_grad_enabled()
        stats_graph = grad and self._stats_in_graph()
        f32 = z.dtype == torch.float32 and params.dtype == torch.float32
        plain = f32 and not (grad and (z.requires_grad or params.requires_grad))
        inference = (arch == "coupling" and plain and not stats_graph
                     and not (params.size(0) > 1 and z.size(1) < 32))
        return arch, (self.D, self.num_stages, self.num_layers, self.num_units), stats_graph, f32, plain, inference

    def _ar_fused_ok(self, z, params, facts=None):
        """[MAF, BatchNorm, Affine] as one kernel: float32, no autograd, shape covered by the MFMA MAF kernel."""
        arch, (D, _, L, U), stats_graph, _, plain, _ = facts or self._facts(z, params)
        return arch == "AR" and plain and not stats_graph and z.dim() == 3 and ops.ar_flow_supported(D, L, U)

    def _ar_train_ok(self, z, params, facts=None):
        """Training through the AR stack with z a constant: one forward kernel, one backward kernel."""
        arch, (D, _, L, U), stats_graph, f32, _, _ = facts or self._facts(z, params)
        return (arch == "AR" and getattr(self, "fused_ar_training", True) and torch.is_grad_enabled()
                and not stats_graph and params.requires_grad and not z.requires_grad and z.dim() == 3 and f32
                and z.size(0) == max(z.size(0), params.size(0))
                and ops.ar_flow_supported(D, L, U) and ops.ar_flow_train_supported(z.size(0), params.size(0), D, L, U))

    def _ar_sample_train_ok(self, z, params, facts=None):
        """One kernel forward, one fused kernel backward for frozen-statistics sampling of the AR stack under autograd
        (csrc/maf_sample_bwd.hip): only with the switch `ar_sample_training` on, float32, grad mode on and params
        requiring grad, constant statistics, a 3-d draw, one parameter row or one per block of samples, exact-f32
        operands, and a shape both kernels cover."""
        arch, (D, _, L, U), stats_graph, f32, _, _ = facts or self._facts(z, params)
        return (getattr(self, "ar_sample_training", False) and arch == "AR" and f32 and torch.is_grad_enabled()
                and params.requires_grad and not stats_graph and z.dim() == 3
                and ops.current_operand_precision() == "fp32"
                and arsample_ops.ar_flow_sample_train_supported(z.size(0), params.size(0), D, L, U))

    def _ar_batch_family(self, z, params, facts):
        """Fresh-statistics sampling of the AR stack as one C call each way (csrc/ar_flow_batch.hip): only with the switch
        `ar_batch_forward` on, float32, a 3-d draw with one block per parameter row, at least two rows in the batch and no
        sample-sharded statistics.  "ar_batch_chain": the call is plain and the forward kernel covers the shape;
        "ar_batch_train": grad mode on, params requiring grad, exact-f32 operands and a shape the sampling backward
        covers too (D <= 32); None: the per-bijector composition.  One measured exclusion (DESIGN.md 22,
        profiles/r18_arbatchbench.txt): without autograd the chain saves launches only, a clear win up to 160,000 values
        in the batch (1.15 .. 1.44 x at 100 x 25 .. 400 samples, D = 4, and 100 x 25 .. 100, D = 16) and a tie from 640,000
        (1.00 .. 1.09 x, the rounds overlap in most runs), so `ar_batch_chain` is offered up to M N D = 160,000 only."""
        _, (D, _, L, U), _, f32, plain, _ = facts
        if not (getattr(self, "ar_batch_forward", False) and f32 and z.dim() == 3 and z.size(0) == params.size(0)
                and z.size(0) * z.size(1) >= 2 and self.batch_stats_reduce is None):
            return None
        if plain:
            small = z.size(0) * z.size(1) * D <= 160000
            return "ar_batch_chain" if small and arbatch_ops.ar_flow_batch_supported(D, L, U) else None
        if (torch.is_grad_enabled() and params.requires_grad and ops.current_operand_precision() == "fp32"
                and arbatch_ops.ar_flow_batch_train_supported(D, L, U)):
            return "ar_batch_train"
        return None

    def _ar_args(self):
        maf, bn = self.bijectors[0], self.bijectors[1]
        mean, alpha = bn._stats_for(None)  # device copies, made once per version of the statistics
        return (maf._masks_for(torch.float32), mean.detach(), alpha.detach(), self.D, self.num_layers, self.num_units)

    def _flow_args(self):
        """The arguments every coupling flow kernel shares: (2S, D) statistics and the shape."""
        mean, alpha = self._bn_stats(_lib.require_device())
        return (mean, alpha, self.D, self.num_stages, self.num_layers, self.num_units)

    def _whole_flow(self):
        """Does the fused coupling path run as ONE kernel (the only one with a fused support stage)?"""
        return ops.resolve_fusion(self.D, self.num_stages, self.num_layers, self.num_units, self.fusion) == _lib.FUSE_FLOW

    def _fused_support(self):
        """The (7, D) device constants of a ToInterval support layer that the one-kernel paths evaluate in
        their load / store stage, or None (no support layer).  Other support layers are not fused: False."""
        if self._n_core == len(self.bijectors):
            return None
        sup = self.bijectors[-1]
        return sup._device_consts() if sup.name == "ToInterval" else False

    def _batch_chain_ok(self, z, params):
        """Shapes of the one-call chains with fresh batch statistics (the narrow MFMA layer kernels)."""
        return (getattr(self, "fused_batch_forward", True) and z.dim() == 3 and z.size(0) == params.size(0)
                and ops.flow_train_supported(z.size(0), params.size(0), 32, self.D, self.num_stages, self.num_layers,
                                             self.num_units))

    def _padded_batch_ok(self, z, params):
        """Shapes of the one-call chains with fresh batch statistics at the embedded width 2H (2 <= D <= 63 but 32,
        num_units <= 16): only with the switch `padded_batch_forward` on, a coupling stack, one parameter row per z row,
        no sample-sharded statistics, and the fusion setting AUTO or FLOW as for the `padded` family."""
        return (getattr(self, "padded_batch_forward", False) and self.arch_type == "coupling" and z.dim() == 3
                and z.size(0) == params.size(0) and self.batch_stats_reduce is None
                and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)
                and padbatch_ops.flow_padded_batch_supported(self.D, self.num_stages, self.num_layers, self.num_units))

    def _context_rows_ok(self, op, z, params, facts, switch):
        """One launch for a per-context call with fewer than 32 samples per context: only with the switch named on, a
        coupling stack, plain, constant statistics, a 3-d z, several parameter rows that are the larger batch, one block
        of z rows for all contexts or one per context (sampling: one per context), the fusion setting AUTO or FLOW as for
        the `padded` family, a shape the `*_supported` function of `_PER_CONTEXT[switch]` covers, and not its measured
        exclusion `slower(op, shape, N)`.  No gradients: calls under autograd keep their routes, or take
        `_context_train_ok`'s families.  `_route` asks twice: `context_rows` (csrc/flow_ctx.hip: one wave per context,
        up to 16 units; ctx_flow_supported, `_context_rows_slower`) and `wide_context_rows` (csrc/flow_ctx_wide.hip: one
        workgroup per context, one layer's operand image resident at a time, 17 <= num_units <= 64; ctx_wide_supported,
        `_context_rows_wide_slower`)."""
        arch, shape, stats_graph, _, plain, _ = facts
        if not (getattr(self, switch, False) and arch == "coupling" and plain and not stats_graph
                and z.dim() == 3 and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)):
            return False
        mod, supported, slower = _PER_CONTEXT[switch]
        M, N = params.size(0), z.size(1)
        if slower(op, shape, N):
            return False
        return M > 1 and z.size(0) in ((M,) if op == "forward" else (1, M)) and getattr(mod, supported)(*shape, N)

    def _context_train_ok(self, z, params, facts, switch):
        """One launch each way for a per-context log_prob under autograd with fewer than 32 samples per context: only
        with the switch named on (independent of every other switch), a coupling stack, float32, grad mode on and params or
        z requiring grad, constant statistics, a 3-d z, several parameter rows that are the larger batch, one block of z
        per context -- or one shared block that requires no grad: its gradient would need a sum over contexts -- the
        fusion setting AUTO or FLOW as for the `padded` family, and a shape the `*_supported` function of
        `_PER_CONTEXT[switch]` covers.  `_route` asks twice: `context_training` (csrc/flow_ctx.hip forward keeping z0,
        csrc/flow_ctx_bwd.hip backward; ctx_train_supported) and `wide_context_training` (csrc/flow_ctx_wide.hip,
        csrc/flow_ctx_wide_bwd.hip; ctx_wide_train_supported).  No measured exclusion in either."""
        arch, shape, stats_graph, f32, _, _ = facts
        if not (getattr(self, switch, False) and arch == "coupling" and f32 and torch.is_grad_enabled()
                and (params.requires_grad or z.requires_grad) and not stats_graph and z.dim() == 3
                and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)):
            return False
        mod, supported, _ = _PER_CONTEXT[switch]
        M = params.size(0)
        return (M > 1 and (z.size(0) == M or (z.size(0) == 1 and not z.requires_grad))
                and getattr(mod, supported)(*shape, z.size(1)))

    def _sample_train_ok(self, z, params, facts):
        """One launch forward, one walk kernel backward for frozen-statistics sampling under autograd
        (csrc/flow_bwd_f16.hip, flow_sample_bwd_kernel): only with the switch `sample_training` on, a coupling stack,
        float32, grad mode on and params requiring grad, constant statistics, a 3-d draw, the fusion setting AUTO or
        FLOW as for the `padded` family, and one parameter row or at least 32 samples per row."""
        arch, shape, stats_graph, f32, _, _ = facts
        return (getattr(self, "sample_training", False) and arch == "coupling" and f32 and torch.is_grad_enabled()
                and params.requires_grad and not stats_graph and z.dim() == 3
                and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)
                and sampletrain_ops.flow_sample_train_supported(z.size(0), params.size(0), z.size(1), *shape))

    def _context_sample_train_ok(self, z, params, facts, switch):
        """One launch each way for frozen-statistics sampling under autograd with several parameter rows and fewer than
        32 draws per row: only with the switch named on (independent of every other switch), a coupling stack, float32,
        grad mode on and params requiring grad, constant statistics, a 3-d draw with one block per parameter row, the
        fusion setting AUTO or FLOW as for the `padded` family, and a shape the `*_supported` function of
        `_PER_CONTEXT[switch]` covers.  `_route` asks twice: `context_sample_training` (csrc/flow_ctx.hip forward,
        csrc/flow_ctx_sample_bwd.hip backward; ctx_sample_supported) and `wide_context_sample_training`
        (csrc/flow_ctx_wide.hip, csrc/flow_ctx_wide_sample_bwd.hip; ctx_wide_sample_supported).  No measured exclusion in
        either: the one of `context_rows_wide` (N = 1 above 48 units) is a measurement of another op and is not copied."""
        arch, shape, stats_graph, f32, _, _ = facts
        if not (getattr(self, switch, False) and arch == "coupling" and f32 and torch.is_grad_enabled()
                and params.requires_grad and not stats_graph and z.dim() == 3
                and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)):
            return False
        mod, supported, _ = _PER_CONTEXT[switch]
        M = params.size(0)
        return M > 1 and z.size(0) == M and getattr(mod, supported)(*shape, z.size(1))

    def _stats_in_graph(self):
        """Do the cached BatchNorm statistics still carry the graph of the batch-mode forward that produced them
        (per-bijector forward under autograd -- the reference's behaviour, bijectors.py:414-415)?  Then every later
        use of them in the same graph must differentiate through them: only the per-bijector composition does."""
        return torch.is_grad_enabled() and any(b.get_last_mean().requires_grad or b.get_last_alpha().requires_grad
                                               for b in self._bn_layers())

    def _fused_ok(self, z, params, facts=None):
        """One-call fused path: coupling stack, float32, no autograd, MFMA-covered shape."""
        _, (D, _, L, U), _, _, _, inference = facts or self._facts(z, params)
        return inference and ops.has_fast_path(D, L, U)

    def _padded_ok(self, z, params, facts=None):
        """One-call whole-flow kernel in its padded layouts (every 2 <= D <= 63 but 32, num_units <= 16): the
        conditions of `_fused_ok`, a 3-d z, and the fusion setting AUTO or FLOW -- FUSE_LAYER keeps the per-layer
        routes of these shapes (the wide chain, or the per-bijector composition)."""
        _, shape, _, _, _, inference = facts or self._facts(z, params)
        return (inference and z.dim() == 3 and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)
                and ops.flow_padded_supported(*shape))

    def _wide_flow_ok(self, op, z, params, facts=None):
        """One-launch whole-flow kernel on the exact-f32 MFMA tile (csrc/flow_wide.hip): only with the switch `wide_flow`
        on, the conditions of `_padded_ok` (coupling, inference, a 3-d z, the fusion setting AUTO or FLOW), and a shape
        wide_flow_supported covers (17 <= num_units <= 64, 2 <= D <= 64, the images of all 2 S layers within the LDS
        budget).  No gradients and no fresh statistics: those calls keep their routes.  One measured exclusion (DESIGN.md
        24, profiles/r20_wideflowbench.txt): sampling with several parameter rows at D % 8 == 0 below 32 stays on the wide
        per-layer chain, which was faster at the one such cell measured (0.92 x at D = 8, S = 1, U = 20, 2,000 rows of 100
        draws: each workgroup's prologue outweighs its seven tiles; 1.13 x at D = 32, S = 4)."""
        if not getattr(self, "wide_flow", False):
            return False
        _, shape, _, _, _, inference = facts or self._facts(z, params)
        if op == "forward" and params.size(0) > 1 and shape[0] % 8 == 0 and shape[0] < 32:
            return False
        return (inference and z.dim() == 3
                and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW) and wideflow_ops.wide_flow_supported(*shape))

    def _wide_flow_stream_ok(self, op, z, params, facts=None):
        """One-launch whole-flow kernel with the layers' operand images streamed through LDS (csrc/flow_wide_stream.hip):
        only with the switch `wide_flow_streamed` on, the conditions of `_wide_flow_ok` (coupling, inference, a 3-d z, the
        fusion setting AUTO or FLOW; no gradients, no fresh statistics), a shape wide_flow_supported does NOT cover --
        so the two families are disjoint whatever the switches say -- and one wide_flow_stream_supported does
        (17 <= num_units <= 64, 2 <= D <= 64, one layer's image within the LDS budget, S <= 1024).  One measured
        exclusion (profiles/r24_widestreambench.txt): at D % 8 == 0, where the switch-off route is the wide
        per-layer chain, the kernel wins every measured cell with one row of up to 2^17 samples in log_prob (1.07 .. 1.68 x
        over four shapes at 2^12 and 2^17) and of 2^12 in sampling (1.06 .. 1.59 x), and loses cells of every other class
        -- sampling, one row of 2^17: 0.98 x at (64, 4, 2, 64); one row of 2^20 samples: 0.76 .. 1.01 x (64, 4, 2, 64:
        0.81 / 0.76); 2,000 rows of 100: 0.75 .. 1.27 x (64, 4, 2, 32: 0.75) -- so D % 8 == 0 is taken only with one block
        of z, one parameter row and N <= 2^17 (forward: N <= 2^12).  Every other D wins all its cells (2.5 .. 11.5 x the
        composition)."""
        if not getattr(self, "wide_flow_streamed", False):
            return False
        _, shape, _, _, _, inference = facts or self._facts(z, params)
        if shape[0] % 8 == 0:  # against the wide per-layer chain: one block of z, one parameter row, N up to the measured win
            if not (z.dim() == 3 and z.size(0) == 1 and params.size(0) == 1 and z.size(1) <= 1 << (12 if op == "forward" else 17)):
                return False
        return (inference and z.dim() == 3 and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)
                and not wideflow_ops.wide_flow_supported(*shape) and widestream_ops.wide_flow_stream_supported(*shape))

    def _train_path(self, z, params, stats_graph=None):
        """The fused training pair of a coupling log_prob: "reversible" (whole-flow forward, one-kernel backward from
        z0), "padded" (the same pair for 2 <= D <= 63 but 32: padded whole-flow forward, the one-kernel backward at the
        embedded width 2H; only with the switch `padded_training` on, and the fusion setting AUTO or FLOW as for the
        `padded` family), "layers" (one fused kernel per layer each way, for the shapes those do not cover) or None."""
        if self._stats_in_graph() if stats_graph is None else stats_graph:
            return None  # the fused training pairs treat the statistics as constants
        shape = (z.size(0), params.size(0), z.size(1), self.D, self.num_stages, self.num_layers, self.num_units)
        if getattr(self, "reversible_training", True) and ops.flow_train_rev_supported(*shape):
            return "reversible"
        if (getattr(self, "padded_training", False) and self.fusion in (_lib.FUSE_AUTO, _lib.FUSE_FLOW)
                and padtrain_ops.flow_padded_train_supported(*shape)):
            return "padded"
        if ops.flow_train_supported(*shape):
            return "layers"
        return None

    def _route(self, op, z, params, freeze_bn=True, f32_draw=False):
        """THE routing decision (table in the module docstring): which kernel family runs `op` ("forward", "log_prob"
        or "inverse") on these tensors.  Pure host logic on the flow's switches and tensor metadata; nothing is
        staged, allocated or launched.  `f32_draw`: the base draw of a "forward" is a float32 tensor, so a
        whole-flow kernel can write log_q itself."""
        arch, _, stats_graph, f32, _, inference = f = self._facts(z, params)
        sup = self.bijectors[-1].name if self._n_core < len(self.bijectors) else None
        interval = sup == "ToInterval"  # the support layer that a one-kernel family evaluates in its load / store stage
        if arch == "affine" or (op == "inverse" and sup is not None):
            return _BIJECTORS
        if arch == "AR":
            if op == "forward" and not freeze_bn:  # fresh batch statistics: one call each way behind `ar_batch_forward`
                family = self._ar_batch_family(z, params, f)
                return Route(family, False, False) if family else _BIJECTORS
            if op != "forward" or interval or sup is None:  # (sampling fuses a ToInterval layer or none)
                if self._ar_fused_ok(z, params, f):
                    return Route("ar_fused", interval, False)
                if op == "log_prob" and self._ar_train_ok(z, params, f):
                    return Route("ar_train", interval, False)
            if op == "forward" and self._ar_sample_train_ok(z, params, f):
                return Route("ar_train_sample", False, False)
            return _BIJECTORS
        # `fused` is asked through the instance: tests switch this family (never `padded`) off with an attribute of it
        forced = vars(self).get("_fused_ok")
        if op == "forward" and not freeze_bn:  # fresh batch statistics
            rows, reduce = z.size(0) * z.size(1), self.batch_stats_reduce is not None
            if ((forced(z, params) if forced else self._fused_ok(z, params, f)) and self._batch_chain_ok(z, params)
                    and (rows > 1 or reduce)):
                return Route("batch_chain", False, False)
            if f32 and not reduce and self._batch_chain_ok(z, params) and rows >= 32:
                return Route("batch_train", False, False)
            if rows > 1 and f32 and self._padded_batch_ok(z, params):  # widths the two above never take
                if inference:
                    return Route("batch_chain_padded", False, False)
                if rows >= 32:
                    return Route("batch_train_padded", False, False)
            return _BIJECTORS
        if self._padded_ok(z, params, f):
            return Route("padded", False, f32_draw)
        if self._wide_flow_ok(op, z, params, f):  # before `fused`: with the switch on it takes D % 8 == 0 from the wide chain
            return Route("wide_flow", False, False)
        if self._wide_flow_stream_ok(op, z, params, f):  # the stage counts `wide_flow` cannot hold: disjoint from it
            return Route("wide_flow_streamed", False, False)
        if forced(z, params) if forced else self._fused_ok(z, params, f):
            whole = (f32_draw or interval) and self._whole_flow()  # the only two that ask
            return Route("fused", interval, f32_draw) if whole else _FUSED
        if op == "log_prob" and f32 and z.dim() == 3 and z.size(0) == max(z.size(0), params.size(0)):
            pair = self._train_path(z, params, stats_graph)
            if pair is not None:
                return Route("train_" + pair, False, False)
        # each per-context predicate is asked twice: up to 16 units, then 17 .. 64 (disjoint shape sets, a switch each)
        if op == "log_prob":
            if self._context_train_ok(z, params, f, "context_training"):
                return Route("train_context", False, False)
            if self._context_train_ok(z, params, f, "wide_context_training"):
                return Route("train_context_wide", False, False)
        if op == "forward":
            if self._sample_train_ok(z, params, f):
                return Route("train_sample", False, f32_draw)
            if self._context_sample_train_ok(z, params, f, "context_sample_training"):
                return Route("train_context_sample", False, False)
            if self._context_sample_train_ok(z, params, f, "wide_context_sample_training"):
                return Route("train_context_sample_wide", False, False)
        # asked last: nothing another family takes changes hands
        if self._context_rows_ok(op, z, params, f, "context_rows"):
            return Route("context_rows", False, False)
        if self._context_rows_ok(op, z, params, f, "wide_context_rows"):
            return Route("context_rows_wide", False, False)
        return _BIJECTORS

    # -- sampling -----------------------------------------------------------
    def __call__(self, N=100, params=None, freeze_bn=False):
        if not self.conditioner:
            return self.forward(self.params, N, freeze_bn=freeze_bn)
        return self.forward(params, N, freeze_bn=freeze_bn)

    def forward(self, params, N=100, freeze_bn=False):
        """Draw N samples per parameter row and their log-density
        (density_estimator.py:364-388).  The base draw is host numpy float64 exactly like
        the reference (so np.random.seed reproduces it); returns z float32 and log_q
        float64 on the parameters' device."""
        M = params.size(0)
        omega = np.random.normal(0.0, 1.0, (M, N, self.D))
        return self._forward_from(omega, params, freeze_bn)

    def sample(self, N=100, params=None, freeze_bn=True, generator=None):
        """Extension (not in the reference): like `forward`, but the base draw comes from the
        device RNG (`torch.randn` on the flow's device, optional `generator`), so no host RNG,
        no float64 staging and no PCIe copy.  Not reproducible against np.random.seed."""
        if not self.conditioner:
            params = self.params
        dev = _lib.require_device()
        omega = torch.randn((params.size(0), N, self.D), device=dev, dtype=torch.float32, generator=generator)
        return self._forward_from(omega, params, freeze_bn)

    def _forward_from(self, omega, params, freeze_bn=False):
        """`forward` with the base draw injected: numpy float64 (M,N,D) like the reference's host
        draw, or a torch tensor (e.g. a device-side torch.randn draw, which skips the host RNG and
        the 8 B/value PCIe copy)."""
        home = params.device
        dev = _lib.require_device()
        p_dev = params if params.device == dev else params.to(dev)
        if torch.is_tensor(omega) and omega.dtype == torch.float32:
            omega64 = None
            z = omega.detach().to(dev)  # device-side draw: no float64 round trip
        else:
            if torch.is_tensor(omega):
                omega64 = omega.detach().to(device=dev, dtype=torch.float64)
            else:
                omega64 = torch.as_tensor(np.ascontiguousarray(omega), dtype=torch.float64).to(dev)
            z = omega64.float()
        route = self._route("forward", z, p_dev, freeze_bn, f32_draw=omega64 is None)
        family, omega_dev = route.family, z
        # the base density of a float32 draw can come out of the whole-flow sampling kernels themselves
        log_q = None if route.writes_log_q else ops.base_log_density_f64(z if omega64 is None else omega64)
        consts = self._fused_support() if route.fuse_support else None
        # sample-sharded batch statistics (self.batch_stats_reduce): the stepwise no-autograd chain exchanges the moments
        # between its launches; every other case -- autograd, other shapes, arch_type "AR" -- runs the per-bijector
        # composition with BatchNorm layers that exchange their moments forward and their gradient sums backward
        # (ops._BnBatchShardedFn).  The one-node training chain computes local moments inside one C call: not offered.
        for b in self._bn_layers():
            b.stats_reduce = None if freeze_bn else self.batch_stats_reduce
        if family == "bijectors":
            # fresh statistics on an AR stack with `ar_sample_training`: the MAF's sampling backward is one kernel for the
            # duration of this call (the decision is recorded on the autograd node, so a later backward keeps it)
            maf = self.bijectors[0] if (self.arch_type == "AR" and getattr(self, "ar_sample_training", False)
                                        and not freeze_bn) else None
            restore = None if maf is None else maf.fused_sampling_backward
            if maf is not None:
                maf.fused_sampling_backward = True
            try:
                idx = 0
                for bijector in self.bijectors[:self._n_core]:
                    if bijector.name == "BatchNorm":
                        z, log_det = bijector(z, use_last=freeze_bn)
                    else:
                        n = bijector.count_num_params()
                        z, log_det = bijector(z, p_dev[:, idx:idx + n])
                        idx += n
                    log_q = log_q - log_det
            finally:
                if maf is not None:
                    maf.fused_sampling_backward = restore
        else:
            written = None
            if family == "ar_fused":
                z, sld = ops.ar_flow_forward_raw(z, p_dev, *self._ar_args(), interval_consts=consts)
            elif family == "ar_train_sample":  # one autograd node, one backward kernel; any support layer runs below
                z, sld = arsample_ops.ar_flow_sample_train(z, p_dev, *self._ar_args())
            elif family == "padded":  # no fused support layer: it runs below as its own kernel
                z, sld, *written = ops.flow_padded_forward_raw(z, p_dev, *self._flow_args(),
                                                               want_log_q=route.writes_log_q)
            elif family in _SAMPLERS:  # one launch (under autograd: each way); the support layer as for `padded`
                mod, name = _SAMPLERS[family]
                z, sld = getattr(mod, name)(z, p_dev, *self._flow_args())
            elif family == "train_sample":  # one autograd node, one backward kernel; the support layer as for `padded`
                z, sld, *written = sampletrain_ops.flow_sample_train(z, p_dev, *self._flow_args(), self.fusion,
                                                                     want_log_q=route.writes_log_q)
            elif family == "fused":  # `written` stays None where the selected kernel variant has no log_q output
                z, sld, *written = ops.flow_forward_raw(z, p_dev, *self._flow_args(), self.fusion, interval_consts=consts,
                                                        want_log_q=route.writes_log_q)
            else:
                # fresh batch statistics in one call for the whole stack -- "batch_chain" without autograd, "batch_train"
                # as one node (gradients through the batch moments included); every BatchNorm layer ends up with the
                # statistics its own forward(use_last=False) would have cached
                bns = self._bn_layers()
                shape = (self.D, self.num_stages, self.num_layers, self.num_units, bns[0].eps)
                if family in ("ar_batch_chain", "ar_batch_train"):  # [MAF, BatchNorm, Affine]: one layer of statistics
                    entry = (arbatch_ops.ar_flow_forward_batch_raw if family == "ar_batch_chain"
                             else arbatch_ops.ar_flow_forward_batch_train)
                    z, sld, mean, alpha = entry(z, p_dev, self.bijectors[0]._masks_for(torch.float32), self.D,
                                                self.num_layers, self.num_units, bns[0].eps)
                    means, alphas = [mean.detach()], [alpha.detach()]
                elif family == "batch_chain":
                    z, sld, means, alphas = ops.flow_forward_batch_raw(z, p_dev, *shape,
                                                                       reduce_moments=self.batch_stats_reduce)
                elif family == "batch_chain_padded":  # ... the same two at 2 <= D <= 63 but 32, at the embedded width
                    z, sld, means, alphas = padbatch_ops.flow_padded_forward_batch_raw(z, p_dev, *shape)
                elif family == "batch_train_padded":
                    z, sld, means, alphas = padbatch_ops.flow_padded_forward_train(z, p_dev, *shape)
                else:
                    z, sld, means, alphas = ops.flow_forward_train(z, p_dev, *shape)
                for i, b in enumerate(bns):
                    b.set_last_stats(means[i], alphas[i])
            if written and written[0] is not None:
                log_q = written[0]
            else:
                log_q = (ops.base_log_density_f64(omega_dev) if log_q is None else log_q) - sld
        if not route.fuse_support:
            for bijector in self.bijectors[self._n_core:]:  # parameter-free support layer (:385-386)
                z, log_det = bijector(z)
                log_q = log_q - log_det
        if home != dev:
            z, log_q = z.to(home), log_q.to(home)
        return z, log_q

    # -- density ------------------------------------------------------------
    def _fused_density(self, family, z, params, consts=None, want_lp=True, want_z0=False, want_sld=False):
        """(log_prob | None, z0 | None, sum_log_det | None) from the one-kernel family named."""
        if family == "ar_fused":
            return ops.ar_flow_log_prob_raw(z, params, *self._ar_args(), want_lp=want_lp, want_z0=want_z0,
                                            want_sld=want_sld, interval_consts=consts)
        if family == "padded":
            return ops.flow_padded_log_prob_raw(z, params, *self._flow_args(), want_lp=want_lp, want_z0=want_z0,
                                                want_sld=want_sld)
        if family in _DENSITIES:
            mod, name = _DENSITIES[family]
            return getattr(mod, name)(z, params, *self._flow_args(), want_lp=want_lp, want_z0=want_z0, want_sld=want_sld)
        return ops.flow_log_prob_raw(z, params, *self._flow_args(), self.fusion, want_lp=want_lp, want_z0=want_z0,
                                     want_sld=want_sld, interval_consts=consts)

    def inverse_and_log_det(self, z, params):
        """Map z back to the base space, accumulating the forward log-dets
        (density_estimator.py:390-406).  Returns (z0, sum_log_det float32 (M,N))."""
        family = self._route("inverse", z, params).family
        if family == "bijectors":
            return self._core_inverse(z, params, self.bijectors)
        return self._fused_density(family, z, params, want_z0=True, want_sld=True, want_lp=False)[1:]

    def _core_inverse(self, z, params, bijectors=None):
        """The reference's loop, one HIP kernel per bijector (the whole stack, or only its
        parameterised core when `bijectors` is None)."""
        if bijectors is None:
            bijectors = self.bijectors[:self._n_core]
        home = z.device
        dev = _lib.require_device()
        if home != dev:
            z = z.to(dev)
        if params.device != dev:
            params = params.to(dev)
        M = max(z.size(0), params.size(0))
        idx = self.D_params
        sum_log_det = torch.zeros((M, z.size(1)), device=dev)
        for bijector in reversed(bijectors):
            n = bijector.count_num_params()
            if n > 0:
                z, log_det = bijector.inverse_and_log_det(z, params[:, idx - n:idx])
                idx -= n
            else:
                z, log_det = bijector.inverse_and_log_det(z)
            sum_log_det = sum_log_det + log_det
        sum_log_det = sum_log_det.float()  # the reference accumulates into a float32 buffer (:394)
        if home != dev:
            z, sum_log_det = z.to(home), sum_log_det.to(home)
        return z, sum_log_det

    def log_prob(self, z, params=None):
        """log q(z) (density_estimator.py:408-416)."""
        if not self.conditioner:
            params = self.params
        family, fuse_support, _ = self._route("log_prob", z, params)
        consts = self._fused_support() if fuse_support else None  # ToInterval^-1 in the kernel's load stage
        ld_support = None
        if self._n_core < len(self.bijectors) and not fuse_support:
            # support layer first (it is the last bijector of the stack), then the core's density:
            # log q(z) = log q_core(s^-1(z)) - log|det ds| -- same sum as density_estimator.py:395-416
            z, ld_support = self.bijectors[-1].inverse_and_log_det(z)
        if family in ("ar_fused", "padded", "fused") or family in _DENSITIES:
            log_q = self._fused_density(family, z, params, consts)[0]
        elif family == "ar_train":
            masks, mean, alpha, D, L, U = self._ar_args()
            log_q = ops.ar_flow_log_prob_train(z, params, masks, mean, alpha, consts, D, L, U)
        elif family == "train_padded":  # ... at 2 <= D <= 63 but 32: the reversible pair at the embedded width
            log_q = padtrain_ops.flow_padded_log_prob_train(z, params, *self._flow_args())
        elif family in _TRAINERS:  # ... per-context rows with fewer than 32 samples each: one launch each way
            mod, name = _TRAINERS[family]
            log_q = getattr(mod, name)(z, params, *self._flow_args())
        elif family != "bijectors":  # training with the BatchNorm statistics constant, one of the two fused pairs
            log_q = ops.flow_log_prob_train(z, params, *self._flow_args(), reversible=family == "train_reversible")
        else:
            z0, sum_log_det = self._core_inverse(z, params)
            log_q = torch.sum(-(z0 ** 2), axis=2) / 2.0 - self.D * np.log(np.sqrt(2.0 * np.pi))
            log_q = log_q - sum_log_det
        return log_q if ld_support is None else log_q - ld_support


def _pos_k(val):
    if val < 1:
        raise ValueError("MoG K %d must be greater than 0." % val)
    return val


MOG_EPS = 1e-12


class MoG(DensityEstimator):
    """Mixture of K Gaussians (density_estimator.py:57-237), on the kernels of csrc/mog_kernels.hip.

    One parameter row is [logits (K) | mu_raw (K, D) | u (K, D(D+1)/2)]: alpha = softmax(logits), U_k upper triangular
    from the packed row-major triangle u with U_ii = exp(u_ii), Sigma_inv_k = U_k^T U_k.  With both `lb` and `ub`
    (length-D arrays; m = (ub - lb)/2, c = (ub + lb)/2): mu = m tanh(mu_raw) + c, U_ii = exp(u_ii)/sqrt(m_i).
    `log_prob` is the reference's formula with its EPS = 1e-12 terms -- for K > 1 it saturates at log EPS = -27.63 --
    evaluated in the log domain, so it is the float64 value of that formula to float32 rounding at every D.  float32 only.

    Sampling: `forward` / `__call__` take their draws from np.random in the fixed order u (M, N), e1, e2 (M, N, D), so
    np.random.seed reproduces a call; component k = #{j : cumsum(alpha)_j <= u}, z = mu_k + U_k^-1 e1 + sqrt(0.001) e2,
    which is the reference's N(mu_k, Sigma_k + 0.001 I) (:152).  One deviation: the log_q beside the samples is this
    class's `log_prob(z, params)` (written by the sampling kernel), where the reference evaluates `log_prob_np`, whose
    only EPS is the one inside the final log.  Samples carry no gradient (the reference detaches there too).

    Extra (not in the reference): `device`, `_forward_from` (injected draws), `sample` (device-side draws)."""

    K = _Checked("K", int, _pos_k)

    def __init__(self, D, conditioner=False, K=1, lb=None, ub=None, device=None):
        super().__init__(D, conditioner)
        self.K = K
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
                else torch.device("cpu")
        self.device = torch.device(device)
        self.count_num_params()
        if not self.conditioner:
            self._param_init()
        self.lb = lb
        self.ub = ub

    def count_num_params(self):
        """density_estimator.py:235-237."""
        self.D_params = self.K * (1 + self.D + self.D * (self.D + 1) // 2)

    def _param_init(self):
        """xavier_normal_ on a (1, D_params) row (:84-88), drawn on the host, then moved, as NormFlow does."""
        init = torch.nn.init.xavier_normal_(torch.zeros(1, self.D_params))
        self.params = init.to(self.device).requires_grad_(True)
        return None

    def _has_bounds(self):
        return (self.lb is not None) and (self.ub is not None)

    def _bounds(self):
        """None, or the (2, D) float32 [lb | ub] block the kernels take (rebuilt when lb / ub were replaced)."""
        if not self._has_bounds():
            return None
        cached = self.__dict__.get("_bounds_cache")
        if cached is None or cached[0] is not self.lb or cached[1] is not self.ub:
            lb, ub = np.asarray(self.lb, dtype=np.float64), np.asarray(self.ub, dtype=np.float64)
            if lb.shape != (self.D,) or ub.shape != (self.D,):
                raise ValueError("MoG lb and ub must have shape (%d,), got %s and %s" % (self.D, lb.shape, ub.shape))
            if not np.all(ub > lb):
                raise ValueError("MoG ub must exceed lb in every dimension.")
            cached = (self.lb, self.ub, torch.tensor(np.stack([lb, ub]), dtype=torch.float32))
            self.__dict__["_bounds_cache"] = cached
        return cached[2]

    def _device_bounds(self):
        """`_bounds()` on the compute device: one copy per device, made once (like ToInterval's constants), so that no
        call copies from the host -- a host copy would synchronise and could not be captured into a HIP graph."""
        dev = _lib.require_device()
        host = self._bounds()
        if host is None:
            return None
        cached = self.__dict__.get("_bounds_dev")
        if cached is None or cached[0] is not host or cached[1] != dev:
            cached = (host, dev, host.to(dev))
            self.__dict__["_bounds_dev"] = cached
        return cached[2]

    def _get_MoG_params(self, params, numpy=False):
        """(alpha (M, K), mu (M, K, D), Sigma_inv (M, K, D, D), Sigma_det (M, K)) as the reference returns them
        (:90-143).  An inspection helper in plain torch ops, in params' dtype and on its device."""
        D, K, T = self.D, self.K, self.D * (self.D + 1) // 2
        M = params.shape[0]
        alpha = torch.softmax(params[:, :K], dim=1)
        mu = params[:, K:K + K * D].reshape(M, K, D)
        raw = params[:, K + K * D:K + K * D + K * T].reshape(M, K, T)
        inds = torch.triu_indices(D, D, device=params.device)
        diag = torch.arange(D, device=params.device)
        U = torch.zeros((M, K, D, D), dtype=params.dtype, device=params.device)
        U[:, :, inds[0], inds[1]] = raw
        u_diag = U[:, :, diag, diag]
        U_exp = torch.exp(u_diag)
        log_det = -2.0 * u_diag
        if self._has_bounds():
            b = self._bounds().to(device=params.device, dtype=params.dtype)
            m, c = (b[1] - b[0]) / 2.0, (b[1] + b[0]) / 2.0
            mu = m * torch.tanh(mu) + c
            U_exp = U_exp / torch.sqrt(m)
            Sigma_det = torch.prod(m * torch.exp(log_det), dim=2)
        else:
            Sigma_det = torch.prod(torch.exp(log_det), dim=2)
        U = U.clone()
        U[:, :, diag, diag] = U_exp
        Sigma_inv = torch.matmul(U.transpose(3, 2), U)
        if numpy:
            alpha = alpha.detach().cpu().numpy()
            alpha = alpha / np.sum(alpha, axis=1)[:, None]
            mu = mu.detach().cpu().numpy()
            Sigma_inv = Sigma_inv.detach().cpu().numpy()
        return alpha, mu, Sigma_inv, Sigma_det

    def _params_or_own(self, params):
        if params is None:
            if self.conditioner:
                raise ValueError("MoG built with conditioner=True needs params.")
            return self.params
        return params

    def log_prob(self, z, params=None):
        """density_estimator.py:172-213: z (M_z, N, D), params (M_p, D_params), M_z and M_p in {1, M} -> (M, N)."""
        return ops.mog_log_prob(z, self._params_or_own(params), self.D, self.K, self._device_bounds())

    def forward(self, params, N=100):
        """density_estimator.py:145-170: (z (M, N, D), log_q (M, N)), float32, on params' device."""
        M = params.size(0)
        u = np.random.uniform(0.0, 1.0, (M, N))
        e1 = np.random.normal(0.0, 1.0, (M, N, self.D))
        e2 = np.random.normal(0.0, 1.0, (M, N, self.D))
        return self._forward_from(torch.as_tensor(u, dtype=torch.float32), torch.as_tensor(e1, dtype=torch.float32),
                                  torch.as_tensor(e2, dtype=torch.float32), params)

    def _forward_from(self, u, e1, e2, params):
        """The sampling map on injected draws: u (M, N) uniform, e1, e2 (M, N, D) standard normal."""
        z, log_q = ops.mog_sample_raw(params.detach(), u, e1, e2, self.D, self.K, self._device_bounds())
        home = params.device
        return (z if z.device == home else z.to(home)), (log_q if log_q.device == home else log_q.to(home))

    def sample(self, N=100, params=None, generator=None):
        """Extension: like `__call__`, with the draws from the device RNG (`generator`: a torch.Generator of the HIP
        device).  Not reproducible against np.random.seed."""
        params = self._params_or_own(params)
        dev = _lib.require_device()
        M = params.size(0)
        u = torch.rand((M, N), device=dev, dtype=torch.float32, generator=generator)
        e = torch.randn((2, M, N, self.D), device=dev, dtype=torch.float32, generator=generator)
        return self._forward_from(u, e[0], e[1], params)

    def log_prob_np(self, z, params):
        """density_estimator.py:215-233 on the host in float64 numpy, without scipy: log(sum_k alpha_k N(z; mu_k,
        Sigma_k) + EPS).  Its only EPS is the one inside the log, so it equals `log_prob` wherever the density is well
        above EPS and differs from it near the floor."""
        z = np.asarray(z.detach().cpu().numpy() if torch.is_tensor(z) else z, dtype=np.float64)
        p = params.detach().cpu().double() if torch.is_tensor(params) else torch.as_tensor(np.asarray(params)).double()
        alpha, mu, Sigma_inv, _ = self._get_MoG_params(p, numpy=True)
        d = z[:, :, None, :] - mu[:, None, :, :]
        q = np.einsum("mnki,mkij,mnkj->mnk", d, Sigma_inv, d)
        _, logdet = np.linalg.slogdet(Sigma_inv)  # log det Sigma_inv = -log det Sigma
        log_n = -0.5 * q + 0.5 * logdet[:, None, :] - 0.5 * self.D * np.log(2.0 * np.pi)
        return np.log(np.sum(alpha[:, None, :] * np.exp(log_n), axis=2) + MOG_EPS)
