#!/usr/bin/env python3
"""One EFN training iteration (efn.train_efn, notebooks/two_network_arch.ipynb cell 5 of the reference) in three forms:

  host    the notebook's structure: host `sample_eta` (float64 numpy) + copy to the device, the eager step, host `KL`
          (copy of z and log_q back, a numpy loop over the contexts)
  device  `sample_eta_device` and `KL_device` (include/tnf_efn.h), the same eager step
  graph   the device form replayed as one HIP graph

The step is the same in all three -- cde.sample(eta, N, freeze_bn=False) with the device base draw, efn_loss, backward,
Adam (capturable) -- so the rows differ by the prior, the KL and the replay alone.  Two configurations: the notebook's
(Dirichlet(5), NormFlow(4, coupling, 1, 1, 15) behind ToSimplex, hidden [100], M = N = 100) and MVN(64) with
NormFlow(64, coupling, 4, 2, 15), M = 64, N = 1024.  Every figure is the median (min .. max) of 20 iterations timed one
by one on the host clock between two synchronisations, after a settling run of 0.3 s.  Then the two new entry points
alone, timed with events: the KL call is its three launches (prepare, stream, reduce) together, so the fraction of the
HBM roof it gives for the stream kernel at 4 (D + 1) B per sample is a lower bound.  `--kernels-only` runs just the KL calls
at the three large shapes, one kernel name per shape: the run to put under `rocprofv3 --kernel-trace --stats` for the
stream kernels' own times.  `--padded-batch-forward` turns NormFlow.padded_batch_forward on for every flow, so that the
notebook's width (D = 4) samples through the one-node chain at the embedded width (include/tnf_padbatch.h), and runs the
iteration forms only; compare with a run without it.
Usage: python tools/efn_train_bench.py [--kernels-only | --padded-batch-forward]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd.exponential_families import efn_loss  # noqa: E402

HBM = 8.0e12  # B/s, the MI355X's nominal HBM3E bandwidth: the roof the fractions below refer to
REPS = 20


def settle(fn, seconds=0.3):
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        fn()
    torch.cuda.synchronize()


def host_clock(fn):
    """median, min, max in ms of REPS calls, each between two synchronisations"""
    settle(fn)
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def event_clock(fn):
    settle(fn)
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def iteration_forms(label, fam, make_flow, hidden, M, N):
    def make():
        """A context network, its optimiser and the two forms of an iteration on them."""
        torch.manual_seed(0)
        np.random.seed(0)
        cde = tnf.ConditionalDensityEstimator(make_flow(), fam.D_eta, hidden)
        opt = torch.optim.Adam(cde.param_net.parameters(), lr=1e-4, capturable=True)
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")

        def step(eta):
            z, log_q = cde.sample(eta, N, freeze_bn=False)
            loss = efn_loss(z, log_q, eta, fam)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach(), z.detach(), log_q.detach()

        def host_form():
            eta = fam.sample_eta(M)
            eta_d = torch.as_tensor(eta, dtype=torch.float32).cuda()
            loss, z, log_q = step(eta_d)
            return loss, float(np.mean(fam.KL(z, log_q, eta)))

        def device_form():
            eta = fam.sample_eta_device(M, seed=0, t_dev=counter)
            counter.add_(1)
            loss, z, log_q = step(eta)
            return loss, torch.mean(fam.KL_device(z, log_q, eta))

        return cde, host_form, device_form

    def host_prior():
        return torch.as_tensor(fam.sample_eta(M), dtype=torch.float32).cuda()

    print("\n%s, M = %d, N = %d: one iteration, median ms (min .. max of %d)" % (label, M, N, REPS), flush=True)
    rows = {}
    # The graph form first, on a network of its own whose every iteration so far ran on the side stream, as in
    # efn.train_efn: the parameters' gradient accumulators remember the stream of their first backward, and a captured
    # backward cannot synchronise with the default stream (see efn.train_efn).
    graph_note = ""
    _, _, device_form = make()
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                device_form()
        torch.cuda.current_stream().wait_stream(side)
        gs = tnf.graphs.GraphedStep(device_form, warmup=0)
        rows["graph"] = host_clock(gs)
        del gs
    except RuntimeError as e:
        graph_note = "graph: capture unavailable (%s)" % str(e).splitlines()[0]
        torch.cuda.synchronize()
    cde, host_form, device_form = make()
    rows["device"] = host_clock(device_form)
    rows["host"] = host_clock(host_form)
    rows["host: sample_eta + copy alone"] = host_clock(host_prior)
    eta_d = fam.sample_eta_device(M)
    with torch.no_grad():
        z_d, lq_d = cde.sample(eta_d, N, freeze_bn=False)
    rows["host: KL alone (copies included)"] = host_clock(lambda: fam.KL(z_d, lq_d, eta_d))
    for name in ("host", "host: sample_eta + copy alone", "host: KL alone (copies included)", "device", "graph"):
        if name in rows:
            print("  %-34s %9.4f ms (%.4f .. %.4f)" % ((name,) + rows[name]), flush=True)
    if graph_note:
        print("  " + graph_note)
    elif rows["graph"][0] > rows["device"][0]:
        print("  NOTE: the graph replay is slower than the eager device form here")
    return rows


def kernels_alone(large_only=False):
    print("\nthe new entry points alone, events, median ms (min .. max of %d)" % REPS)
    for fam, M in () if large_only else ((tnf.Dirichlet(5), 100), (tnf.MVN(5), 100), (tnf.MVN(64), 64), (tnf.MVN(64), 1024)):
        med, lo, hi = event_clock(lambda: fam.sample_eta_device(M))
        print("  sample_eta_device %-9s D=%-2d M=%-5d %9.4f ms (%.4f .. %.4f)"
              % (type(fam).__name__, fam.D, M, med, lo, hi))
    for fam, M, N in ((tnf.Dirichlet(5), 100, 100), (tnf.Dirichlet(5), 100, 1 << 18), (tnf.MVN(5), 100, 1 << 18),
                      (tnf.MVN(64), 64, 1024), (tnf.MVN(64), 64, 1 << 16)):
        if large_only and N < 1 << 16:
            continue
        eta = fam.sample_eta_device(M)
        if type(fam) is tnf.Dirichlet:
            z = torch.rand(M, N, fam.D, device="cuda")
            z = z / z.sum(dim=2, keepdim=True)
        else:
            z = torch.randn(M, N, fam.D, device="cuda")
        lq = torch.randn(M, N, device="cuda", dtype=torch.float64)
        med, lo, hi = event_clock(lambda: fam.KL_device(z, lq, eta))
        byts = 4 * (fam.D + 1)
        print("  KL_device         %-9s D=%-2d M=%-5d N=%-7d %9.4f ms (%.4f .. %.4f)  %9.1f M samples/s  >= %5.1f %% of the "
              "HBM roof at %d B/sample" % (type(fam).__name__, fam.D, M, N, med, lo, hi, M * N / med / 1e3,
                                           100 * M * N * byts / (med * 1e-3) / HBM, byts))
        del z, lq


if __name__ == "__main__":
    print("device: %s" % torch.cuda.get_device_name(0))
    if sys.argv[1:] == ["--kernels-only"]:
        kernels_alone(large_only=True)
        sys.exit(0)
    padded = sys.argv[1:] == ["--padded-batch-forward"]
    if padded:
        tnf.NormFlow.padded_batch_forward = True
        print("NormFlow.padded_batch_forward = True")
    iteration_forms("notebook: Dirichlet(5), NormFlow(4, True, 'coupling', 1, 1, 15, ToSimplex(4)), hidden [100]",
                    tnf.Dirichlet(5), lambda: tnf.NormFlow(4, True, "coupling", 1, 1, 15, support_layer=tnf.ToSimplex(4)),
                    [100], 100, 100)
    iteration_forms("MVN(64), NormFlow(64, True, 'coupling', 4, 2, 15), hidden [100]", tnf.MVN(64),
                    lambda: tnf.NormFlow(64, True, "coupling", 4, 2, 15), [100], 64, 1024)
    if not padded:
        kernels_alone()
