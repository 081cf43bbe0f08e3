"""The N > 1 path on CPU: world_size-2 gloo processes exercise the sample sharding, the
ragged all-gather, the one-bucket gradient all-reduce and the BatchNorm moment exchange of
torch_nf_amd/distributed.py.  The per-shard arithmetic is injected (the CPU oracle stands in
for the HIP kernels, which need a GPU); what is under test is the distributed plumbing."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

D, S, L, U, N = 8, 1, 2, 15, 37  # odd N -> ragged shards


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(seed=0):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import flow_oracle as orc

    rng = np.random.RandomState(seed)
    params = torch.tensor(rng.normal(0, 0.1, (1, orc.flow_num_params(D, S, L, U)))).float()
    stats = [(torch.tensor(rng.normal(0, 0.3, D)).float(), torch.tensor(np.exp(rng.normal(0, 0.2, D))).float())
             for _ in range(2 * S)]
    z = torch.tensor(rng.normal(0, 1, (1, N, D))).float()
    return orc, params, stats, z


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch_nf_amd import distributed as tdist

        orc, params, stats, z = _setup()
        torch.set_num_threads(1)
        z_local = tdist.shard_samples(z)
        lo, hi = tdist.shard_bounds(N, world, rank)
        assert z_local.shape[1] == hi - lo

        # 1. density evaluation shards with no collective; gather only to compare
        fn = lambda zz: orc.flow_log_prob(zz, params, D, S, L, U, stats)
        lp_all = tdist.sharded_log_prob(fn, z_local, gather=True)
        full = fn(z)
        assert lp_all.shape == full.shape
        torch.testing.assert_close(lp_all, full, rtol=1e-6, atol=1e-6)

        # 2. training step: per-rank loss on the local shard, ONE all-reduce of the flat gradient
        p = params.clone().requires_grad_()
        loss_local = -orc.flow_log_prob(z_local, p, D, S, L, U, stats).sum() / N
        loss_local.backward()
        tdist.allreduce_gradients([p])
        p_full = params.clone().requires_grad_()
        (-orc.flow_log_prob(z, p_full, D, S, L, U, stats).mean()).backward()
        torch.testing.assert_close(p.grad, p_full.grad, rtol=1e-5, atol=1e-7)

        # 3. batch-statistics BatchNorm across shards: global moments from per-rank sums
        zl = z_local.reshape(-1, D).double()
        n, mean, var_b = tdist.allreduce_moments(torch.tensor(float(zl.shape[0])), zl.sum(0), (zl * zl).sum(0))
        zf = z.reshape(-1, D).double()
        assert int(n.item()) == N
        torch.testing.assert_close(mean, zf.mean(0), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(var_b, zf.var(0, unbiased=False), rtol=1e-10, atol=1e-12)
        out.put((rank, "ok"))
    except Exception as e:  # surface the failure in the parent
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


# ---------------------------------------------------------------------------
# The exchange sequence of a sample-sharded batch-statistics forward (SURVEY 8e bullet 3): ops.run_batch_steps drives
# begin / layer / all-reduce of the moments / fold / end.  On the GPU the steps are the C ABI
# (ops.FlowForwardBatchSteps, tests/test_gpu_parity.py::test_batch_stats_forward_sharded_steps); here the same driver
# and the same reducer (distributed.moment_reducer over gloo) run over an oracle-backed stand-in for the kernels, and
# the two ranks' shards must reproduce the single-process forward with full-batch statistics.
# ---------------------------------------------------------------------------
class _OracleSteps:
    """The FlowForwardBatchSteps protocol over the CPU oracle (one coupling layer per step; the BatchNorm (+ Affine)
    behind it is applied in the next layer's load stage / in end(), from the moments as they are at fold time)."""

    def __init__(self, orc, omega, params, eps=1e-5):
        self.orc, self.params, self.eps = orc, params, eps
        self.n_layers = 2 * S
        self.z = torch.tensor(omega).float()
        self.log_q = torch.tensor(orc.base_log_density_f64(omega))
        self.layout = [(k, n, up) for k, n, up in orc.flow_layout(D, S, L, U)]
        self.pending = None  # (mean, alpha) of the BatchNorm behind the last layer
        self.stats = []

    def begin(self):
        self.offsets, off = [], 0
        for kind, n, up in self.layout:
            self.offsets.append(off)
            off += n

    def _apply_pending(self, c_prev):
        mean, alpha = self.pending
        self.z, ld = self.orc.bn_forward_frozen(self.z, mean, alpha)
        self.log_q = self.log_q - ld
        if c_prev & 1:  # the Affine that closes a stage
            i = [j for j, (k, _, _) in enumerate(self.layout) if k == "affine"][c_prev >> 1]
            n = self.layout[i][1]
            self.z, ld = self.orc.affine(self.z, self.params[:, self.offsets[i]:self.offsets[i] + n], D, False)
            self.log_q = self.log_q - ld

    def layer(self, c):
        if c > 0:
            self._apply_pending(c - 1)
        i = [j for j, (k, _, _) in enumerate(self.layout) if k == "coupling"][c]
        kind, n, up = self.layout[i]
        self.z, ld = self.orc.coupling(self.z, self.params[:, self.offsets[i]:self.offsets[i] + n], D, L, U, up, False)
        self.log_q = self.log_q - ld
        rows = self.z.reshape(-1, D).double()
        self.moments = torch.cat([rows.sum(0), (rows * rows).sum(0), torch.tensor([float(rows.shape[0])]).double()])
        return self.moments

    def fold(self, c):
        n = self.moments[2 * D]
        mean = self.moments[:D] / n
        var_b = (self.moments[D:2 * D] / n - mean * mean).clamp_min(0.0)
        self.pending = (mean.float(), torch.sqrt(var_b + self.eps).float())
        self.stats.append(self.pending)

    def end(self):
        self._apply_pending(self.n_layers - 1)
        return self.z, self.log_q, self.stats


def _worker_steps(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch_nf_amd import distributed as tdist
        from torch_nf_amd import ops

        orc, params, _, _ = _setup(3)
        torch.set_num_threads(1)
        omega = np.random.RandomState(11).normal(0, 1, (1, N, D))
        lo, hi = tdist.shard_bounds(N, world, rank)
        z_l, lq_l, stats_l = ops.run_batch_steps(_OracleSteps(orc, omega[:, lo:hi], params), tdist.moment_reducer())
        z_full, lq_full, stats_full = orc.flow_forward(omega, params, D, S, L, U, None)
        torch.testing.assert_close(z_l, z_full[:, lo:hi], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lq_l, lq_full[:, lo:hi], rtol=1e-6, atol=1e-4)
        for (m, a), (mf, af) in zip(stats_l, stats_full):
            torch.testing.assert_close(m, mf, rtol=1e-5, atol=1e-6)
            torch.testing.assert_close(a, af, rtol=1e-5, atol=1e-6)
        # without the exchange the shard's own statistics differ (the test would be vacuous otherwise)
        z_loc, _, _ = ops.run_batch_steps(_OracleSteps(orc, omega[:, lo:hi], params), None)
        assert (z_loc - z_full[:, lo:hi]).abs().max() > 1e-3
        out.put((rank, "ok"))
    except Exception as e:
        out.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sharded_batch_statistics():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_steps, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


class _TorchBnKernels:
    """CPU stand-ins for ops.HipBnShardKernels (the four halves of the sample-sharded batch-statistics BatchNorm)."""

    @staticmethod
    def moments(z):
        rows = z.reshape(-1, z.shape[-1]).double()
        return torch.cat([rows.sum(0), (rows * rows).sum(0), torch.tensor([float(rows.shape[0])]).double()])

    @staticmethod
    def normalize(z, mom, eps):
        d = z.shape[-1]
        n = mom[2 * d]
        mean = mom[:d] / n
        alpha = torch.sqrt((mom[d:2 * d] / n - mean * mean).clamp_min(0.0) + eps)
        return ((z.double() - mean) / alpha).float(), -torch.log(alpha).sum().float(), mean.float(), alpha.float()

    @staticmethod
    def backward_sums(zn, g):
        d = zn.shape[-1]
        return torch.cat([g.reshape(-1, d).double().sum(0), (g * zn).reshape(-1, d).double().sum(0)])

    @staticmethod
    def backward_apply(zn, g, g_ld, alpha, sums, count):
        d = zn.shape[-1]
        gl = 0.0 if g_ld is None else g_ld.double()
        return ((g.double() - sums[:d] / count - zn.double() * (sums[d:] + gl) / count) / alpha.double()).float()


def _bn_loss(zn, ld, mean, alpha, w, z2, w2):
    # the normalised rows, the log-det, and a LATER use of the cached statistics (an inverse on other data) in one graph
    return (zn * w).sum() + 0.7 * ld + ((z2 * alpha + mean) * w2).sum()


def _worker_bn_autograd(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch_nf_amd import distributed as tdist
        from torch_nf_amd import ops

        torch.set_num_threads(1)
        rng = np.random.RandomState(5)
        z = torch.tensor(rng.normal(0.3, 1.7, (2, N, D))).float()
        w = torch.tensor(rng.normal(0, 1, (2, N, D))).float()
        z2 = torch.tensor(rng.normal(0, 1, (2, N, D))).float()
        w2 = torch.tensor(rng.normal(0, 1, (2, N, D))).float()
        lo, hi = tdist.shard_bounds(N, world, rank)
        # single-process reference: plain torch autograd through the statistics of the WHOLE batch, the loss summed over
        # the shards exactly as the ranks sum theirs
        zf = z.clone().requires_grad_()
        rows = zf.reshape(-1, D)
        mean = rows.mean(0)
        alpha = torch.sqrt(rows.var(0, unbiased=False) + 1e-5)
        zn = (zf - mean) / alpha
        ld = -torch.log(alpha).sum()
        total = 0.0
        for r in range(world):
            a, b = tdist.shard_bounds(N, world, r)
            total = total + _bn_loss(zn[:, a:b], ld, mean, alpha, w[:, a:b], z2[:, a:b], w2[:, a:b])
        total.backward()
        # this rank: its rows only, the exchange through the real reducer
        zl = z[:, lo:hi].clone().requires_grad_()
        zn_l, ld_l, mean_l, alpha_l = ops.bn_batch_forward_sharded(zl, 1e-5, tdist.moment_reducer(), _TorchBnKernels)
        torch.testing.assert_close(zn_l, zn[:, lo:hi].detach(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(alpha_l, alpha.detach(), rtol=1e-6, atol=1e-6)
        _bn_loss(zn_l, ld_l, mean_l, alpha_l, w[:, lo:hi], z2[:, lo:hi], w2[:, lo:hi]).backward()
        torch.testing.assert_close(zl.grad, zf.grad[:, lo:hi], rtol=2e-4, atol=2e-5)
        # without the exchange the gradient differs (the test is not vacuous)
        zl2 = z[:, lo:hi].clone().requires_grad_()
        o = ops.bn_batch_forward_sharded(zl2, 1e-5, lambda t: t, _TorchBnKernels)
        _bn_loss(*o, w[:, lo:hi], z2[:, lo:hi], w2[:, lo:hi]).backward()
        assert (zl2.grad - zf.grad[:, lo:hi]).abs().max() > 1e-3
        out.put((rank, "ok"))
    except Exception as e:
        import traceback

        out.put((rank, repr(e) + traceback.format_exc()[-400:]))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sharded_batch_statistics_with_gradients():
    """VERDICT r2 #7a: batch statistics of a sample-sharded batch UNDER AUTOGRAD -- moments all-reduced forward, the
    gradient sums (and the gradients of the replicated statistics) all-reduced backward -- against the single-process
    gradient (bijectors.py:401-415 differentiates through the statistics of the whole batch)."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_bn_autograd, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


class _GaussCde:
    """CPU stand-in for ConditionalDensityEstimator in the driver tests: q(z | x) = N(mu(x), diag(sigma(x)^2)) with
    (mu, log sigma) = param_net(x).  Same call surface as the product class (param_net, log_prob, __call__, sample)."""

    def __init__(self, Dz, Dx, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.Dz = Dz
        self.param_net = torch.nn.Sequential(torch.nn.Linear(Dx, 16), torch.nn.Tanh(), torch.nn.Linear(16, 2 * Dz))
        for p in self.param_net.parameters():
            p.data = 0.3 * torch.randn(p.shape, generator=g)

    def log_prob(self, z, x):
        out = self.param_net(x)
        mu, ls = out[:, None, :self.Dz], out[:, None, self.Dz:].clamp(-3, 3)
        return (-0.5 * ((z - mu) / torch.exp(ls)) ** 2 - ls - 0.9189385).sum(-1)

    def __call__(self, x, N=100, freeze_bn=True):
        out = self.param_net(x)
        mu, ls = out[:, None, :self.Dz], out[:, None, self.Dz:].clamp(-3, 3)
        z = mu + torch.exp(ls) * torch.randn(x.shape[0], N, self.Dz)
        return z, self.log_prob(z, x)

    sample = __call__


def _worker_apt(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torch_nf_amd import distributed as tdist
        from torch_nf_amd import lfi, systems

        torch.set_num_threads(1)
        mat = systems.Mat(2)
        x0 = np.array([[0.5, 1.0]])
        # 1. one step by hand: shard losses, ONE averaged all-reduce == the gradient of the mean of the shard losses
        rng = np.random.RandomState(2)
        zb = torch.tensor(rng.uniform(-2, 2, (32, mat.D))).float()
        xb = torch.tensor(mat.simulate(zb.numpy())).float()
        lpb = mat.log_prior(zb)
        atoms = lfi._atom_indices(16, 5, torch.device("cpu"), generator=torch.Generator().manual_seed(7))
        cde = _GaussCde(mat.D, 2, seed=1)
        sl = slice(16 * rank, 16 * rank + 16)
        lfi.apt_loss(cde, zb[sl], xb[sl], lpb[sl], atoms).backward()
        tdist.allreduce_gradients(list(cde.param_net.parameters()), average=True)
        ref = _GaussCde(mat.D, 2, seed=1)
        (0.5 * (lfi.apt_loss(ref, zb[:16], xb[:16], lpb[:16], atoms) + lfi.apt_loss(ref, zb[16:], xb[16:], lpb[16:], atoms))).backward()
        for a, b in zip(cde.param_net.parameters(), ref.param_net.parameters()):
            torch.testing.assert_close(a.grad, b.grad, rtol=1e-5, atol=1e-6)
        # 2. the drivers end to end: ranks start from DIFFERENT networks (rank 0's is broadcast), simulate disjoint slices,
        #    and must hold bit-identical networks afterwards
        np.random.seed(0)
        torch.manual_seed(100 + rank)
        cde = _GaussCde(mat.D, 2, seed=10 + rank)
        cde, losses, zs, lps, _ = lfi.train_APT(cde, mat, x0, M=32, M_atom=6, R=2, num_iters=25, num_sims=120, lr=5e-3)
        assert losses.shape == (50,) and np.isfinite(losses).all() and len(zs) == 2
        assert losses[-10:].mean() < losses[:10].mean()
        flat = torch.cat([p.detach().reshape(-1) for p in cde.param_net.parameters()])
        both = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1])
        cde2 = _GaussCde(mat.D, 2, seed=20 + rank)
        l2 = lfi.train_SNPE(cde2, mat, x0, M=32, R=2, num_iters=20, num_sims=120, lr=5e-3)
        assert l2.shape == (40,) and np.isfinite(l2).all()
        flat = torch.cat([p.detach().reshape(-1) for p in cde2.param_net.parameters()])
        both = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(both, flat)
        assert torch.equal(both[0], both[1])
        out.put((rank, "ok"))
    except Exception as e:
        import traceback

        out.put((rank, repr(e) + traceback.format_exc()[-600:]))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_data_parallel_lfi_drivers():
    """VERDICT r2 #7b: lfi.train_APT / train_SNPE data-parallel (BASELINE configs[4] needs the LFI script on the GPUs of
    one node): simulations and contexts sharded over the ranks, ONE averaged gradient all-reduce per step, models
    bit-identical across ranks afterwards.  The density is a CPU stand-in (the flow kernels need a GPU); the simulator
    (systems.Mat), the drivers and the collectives are the product's."""
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_apt, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(0, "ok"), (1, "ok")], results


def test_bench_launcher_dry_run():
    """`python bench.py --gpus N` (not under torch.distributed.run) starts its N ranks itself as a CHILD process
    group; the dry run prints that command without touching a GPU or starting anything."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "7", "--warmup", "2",
                          "--dry-run-launcher"], capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    cmd = json.loads(res.stdout.strip().splitlines()[-1])["launcher"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")):]
    assert tail[1:] == ["--gpus", "8", "--steps", "7", "--warmup", "2"]


def test_bench_launcher_dry_run_forwards_full():
    """--full and the options that only act with it reach every rank of the self-launched group."""
    import json
    import subprocess

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--no-extras", "--dry-run-launcher"],
                         capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stderr
    cmd = json.loads(res.stdout.strip().splitlines()[-1])["launcher"]
    tail = cmd[cmd.index(os.path.join(ROOT, "bench.py")):]
    assert tail[1:] == ["--gpus", "2", "--steps", "7", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-extras"]
