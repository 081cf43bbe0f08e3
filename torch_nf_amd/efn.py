"""Training loop of an exponential family network (EFN): `train_efn` of the reference's
notebooks/two_network_arch.ipynb (cell 5), restated with the whole iteration on the device.

The notebook's loop draws eta on the host (`exp_fam.sample_eta`, float64 numpy, two matrix inversions for MVN), draws the
flow's base noise with np.random.normal, and copies every sample back to the host for `exp_fam.KL`, a Python loop over the
contexts: two synchronisations per iteration.  Here the prior and the KL are HIP kernels (include/tnf_efn.h), the base
draw comes from the device RNG, and an iteration is some dozens of launches with no host round trip, so it is replayed as
one HIP graph.

Deviations from the notebook, all deliberate:
  * eta comes from the counter-based stream of include/tnf_efn.h keyed by `seed` (draw index = iteration), the base noise
    from torch's device generator (torch.manual_seed governs it): the same distributions, not np.random's stream;
  * the notebook stops at the first iteration whose eta, z or log_prob is not finite, before that iteration's update.
    Looking costs a synchronisation, so the loop looks every `check_every` iterations and returns arrays that end before
    the first such iteration; the iterations that ran in between have updated the parameters, and are not rolled back."""
import numpy as np
import torch

from .bijectors import ToSimplex
from .exponential_families import ExponentialFamily, efn_loss


def _flow_width(de):
    """The width of the samples a density estimator returns: D, or D + 1 behind a ToSimplex support layer."""
    return de.D + 1 if isinstance(getattr(de, "support_layer", None), ToSimplex) else de.D


def train_efn(cde, exp_fam, M=100, N=100, num_iters=1000, lr=1e-4, seed=0, prior_kwargs=None, use_graph=None,
              check_every=100, verbose=False):
    """Train `cde` (a ConditionalDensityEstimator whose context is eta) so that cde(eta) approximates the member eta of
    the exponential family `exp_fam`, for eta drawn from the family's prior.  Every iteration:

        eta = exp_fam.sample_eta_device(M, seed=seed, t_dev=counter, **prior_kwargs);  counter += 1   (on the device)
        z, log_q = cde.sample(eta, N, freeze_bn=False)
        loss = efn_loss(z, log_q, eta, exp_fam) = mean(log_q - eta . T(z));  zero_grad, backward, Adam
        KL = mean(exp_fam.KL_device(z, log_q, eta))

    :param M: contexts (draws of eta) per iteration.  :param N: samples per context.
    :param prior_kwargs: hyper-parameters of the prior, as `sample_eta` takes them (sigma_mu, iw_df_fac; lb, ub).
    :param use_graph: replay the iteration as one HIP graph (graphs.GraphedStep, Adam with capturable=True); default:
        on a HIP device.  Three real iterations run on a side stream before the capture and count among num_iters; an
        iteration that cannot be captured is no error: the remaining ones run eagerly.
    :param check_every: look for a non-finite eta / z / log_q every this many iterations (see the module docstring).
    :return: (losses, KLs), numpy arrays of the completed iterations."""
    for name, v in (("M", M), ("N", N), ("num_iters", num_iters), ("check_every", check_every)):
        if type(v) is not int or v < 1:
            raise ValueError("train_efn: %s must be a positive int, got %r" % (name, v))
    if not isinstance(exp_fam, ExponentialFamily) and not (hasattr(exp_fam, "sample_eta_device")
                                                           and hasattr(exp_fam, "KL_device")):
        raise ValueError("train_efn: exp_fam must draw and score on the device (sample_eta_device, KL_device), got %s"
                         % type(exp_fam).__name__)
    width = _flow_width(cde.density_estimator)
    if width != exp_fam.D:
        raise ValueError("train_efn: the flow returns samples of width %d, the family has D=%d" % (width, exp_fam.D))
    if cde.D_x != exp_fam.D_eta:
        raise ValueError("train_efn: param_net takes contexts of width D_x=%d, the family has D_eta=%d"
                         % (cde.D_x, exp_fam.D_eta))
    prior_kwargs = dict(prior_kwargs or {})
    dev = next(cde.param_net.parameters()).device
    if use_graph is None:
        use_graph = dev.type == "cuda"
    # capturable on a HIP device in both modes: the eager and the graphed run then take the same Adam arithmetic
    opt = torch.optim.Adam(cde.param_net.parameters(), lr=lr, capturable=dev.type == "cuda")
    counter = torch.zeros(1, dtype=torch.int64, device=dev)  # the draw index of the prior's stream

    def step():
        eta = exp_fam.sample_eta_device(M, seed=seed, t_dev=counter, **prior_kwargs)
        counter.add_(1)
        z, log_q = cde.sample(eta, N, freeze_bn=False)
        loss = efn_loss(z, log_q, eta, exp_fam)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        z, log_q = z.detach(), log_q.detach()
        kl = torch.mean(exp_fam.KL_device(z, log_q, eta))
        finite = torch.isfinite(eta).all() & torch.isfinite(z).all() & torch.isfinite(log_q).all()
        return loss.detach(), kl, finite

    rows = []  # (loss, KL, finite) of every iteration run so far, on the device
    checked = 0

    def first_bad():
        """Index of the first non-finite iteration among the unchecked ones, or None: the loop's only synchronisation."""
        nonlocal checked
        if checked == len(rows):
            return None
        bad = (~torch.stack([r[2] for r in rows[checked:]])).nonzero()
        first = checked + int(bad[0]) if bad.numel() else None
        checked = len(rows)
        return first

    def run(fn, count):
        """`count` iterations of fn -> True when a non-finite one ended the run."""
        for _ in range(count):
            rows.append(tuple(o.clone() for o in fn()))
            if len(rows) % check_every == 0 or len(rows) == num_iters:
                first = first_bad()
                if first is not None:
                    del rows[first:]
                    return True
                if verbose:
                    print("%d: loss=%.2E, KL=%.2E" % (len(rows), float(rows[-1][0]), float(rows[-1][1])))
        return False

    stopped = False
    if use_graph and num_iters > 4:
        from .graphs import GraphedStep

        # The per-bijector sampling path leaves its BatchNorm layers holding statistics that carry the autograd graph of
        # the last call (bijectors.py:414-415 of the reference), and with it the parameters' gradient accumulators, which
        # remember the stream of their first backward.  If that was the default stream -- a cde that has been trained
        # eagerly before this call -- the captured backward would have to synchronise with the default stream, which a
        # capture cannot do.  Dropping that graph here makes the warm-up below create them anew on its side stream.
        for b in getattr(cde.density_estimator, "_bn_layers", list)():
            b.set_last_stats(b.get_last_mean(), b.get_last_alpha())
        side = torch.cuda.Stream()  # three real iterations on a side stream before the capture
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            stopped = run(step, 3)
        torch.cuda.current_stream().wait_stream(side)
        if not stopped:
            try:
                gs = GraphedStep(step, warmup=0)
            except RuntimeError as e:  # an iteration this device / build cannot capture: finish eagerly
                gs = None
                if verbose:
                    print("graph capture unavailable (%s), running eagerly" % str(e).splitlines()[0])
                torch.cuda.synchronize()
            if gs is not None:
                stopped = run(gs, num_iters - len(rows))
    if not stopped:
        run(step, num_iters - len(rows))
    if not rows:
        return np.zeros(0), np.zeros(0)
    losses = torch.stack([r[0] for r in rows]).double().cpu().numpy()
    KLs = torch.stack([r[1] for r in rows]).double().cpu().numpy()
    return losses, KLs
