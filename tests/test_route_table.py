"""Which kernel family runs each NormFlow call: a fixed grid of calls against tests/route_table.json.

The harness knows nothing of how NormFlow chooses.  It replaces `_lib.require_device` (the CPU stands in for the
device) and every entry of `torch_nf_amd.ops` that density_estimator.py or bijectors.py can reach.  A support-layer op
and `base_log_density_f64` note their name and return tensors of the right shape, so the call goes on; every other
entry notes its name with the route-relevant arguments and raises a private sentinel.  The noted sequence -- or the
type of any other exception -- is the call's trace.  Only `ops` is patched, so this file runs unchanged on any
commit: `python tests/test_route_table.py --write` records the table (done once, on the commit whose routing is to
be preserved; the table is not regenerated afterwards).  Needs the built library for the tnf_*_supported predicates
only; no GPU."""
import contextlib
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch_nf_amd as tnf  # noqa: E402
from torch_nf_amd import _lib, ops  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "route_table.json")
L = 2  # num_layers of every flow of the grid


class _Reached(Exception):
    """A recorder of a kernel entry ends the call here."""


CONTINUE = ("base_log_density_f64", "to_interval", "to_simplex")
STOP = ("flow_log_prob_raw", "flow_forward_raw", "flow_padded_log_prob_raw", "flow_padded_forward_raw",
        "ar_flow_log_prob_raw", "ar_flow_forward_raw", "ar_flow_log_prob_train", "flow_log_prob_train",
        "flow_forward_batch_raw", "flow_forward_train", "coupling", "affine", "bn_apply", "bn_batch_forward", "maf")
NOTED = ("fusion", "want_lp", "want_z0", "want_sld", "want_log_q", "reversible")
NOTED_IS_NONE = ("interval_consts", "reduce_moments")
FAMILY = {"ar_flow_log_prob_raw": "ar_fused", "ar_flow_forward_raw": "ar_fused", "ar_flow_log_prob_train": "ar_train",
          "flow_padded_log_prob_raw": "padded", "flow_padded_forward_raw": "padded", "flow_log_prob_raw": "fused",
          "flow_forward_raw": "fused", "flow_log_prob_train(reversible=True)": "train_reversible",
          "flow_log_prob_train(reversible=False)": "train_layers", "flow_forward_batch_raw": "batch_chain",
          "flow_forward_train": "batch_train", "coupling": "bijectors", "affine": "bijectors", "maf": "bijectors",
          "bn_apply": "bijectors", "bn_batch_forward": "bijectors"}
FAMILIES = sorted(set(FAMILY.values()))


def _stand_in(name, z):
    """What a pass-through op returns: same dtype and autograd state as the real one, zeros for the log-det."""
    if name == "base_log_density_f64":
        return torch.zeros(z.shape[:2], dtype=torch.float64)
    ld = (z * 0).sum(-1)
    return (torch.cat((z, z[..., :1]), -1) if name == "to_simplex" else z + 0), ld


@contextlib.contextmanager
def recording(trace):
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "require_device", lambda: torch.device("cpu"))
        for name in CONTINUE + STOP:
            sig = inspect.signature(getattr(ops, name))

            def recorder(*args, _name=name, _sig=sig, **kwargs):
                bound = _sig.bind(*args, **kwargs)
                bound.apply_defaults()
                a = bound.arguments
                if _name in CONTINUE:
                    trace.append(_name)
                    return _stand_in(_name, args[0])
                noted = ["%s=%s" % (k, a[k]) for k in NOTED if k in a]
                noted += ["%s_is_none=%s" % (k, a[k] is None) for k in NOTED_IS_NONE if k in a]
                trace.append("%s(%s)" % (_name, ",".join(noted)) if noted else _name)
                raise _Reached()

            mp.setattr(ops, name, recorder)
        yield


# ---- the grid --------------------------------------------------------------------------------------------------------
DEFAULTS = dict(op="log_prob", arch="coupling", D=64, U=15, S=4, sup=None, fusion="AUTO", rows="one", M=1, N=64,
                draw="numpy64", freeze_bn=True, zdim=3, zdtype="float32", p_grad=False, z_grad=False, no_grad=False,
                stats_graph=False, off=None, reduce=False, override=False)


def row(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def row_id(r):
    return " ".join("%s=%s" % (k, r[k]) for k in DEFAULTS if k == "op" or r[k] != DEFAULTS[k])


def _grid():
    g = []
    shapes = [dict(M=1, N=64), dict(M=3, N=32, rows="M"), dict(M=3, N=31, rows="M"), dict(M=4, N=1, rows="M"),
              dict(M=1, N=1), dict(M=3, N=31), dict(M=3, N=32)]
    ops_ = [dict(op="log_prob"), dict(op="inverse"), dict(op="forward"), dict(op="forward", freeze_bn=False)]
    # every shape of the catalogue, every architecture, no autograd and training
    for o in ops_:
        for arch in ("coupling", "AR", "affine"):
            for D in (2, 5, 16, 32, 33, 48, 64):
                for U in (15, 16, 20):
                    for S in (1, 4):
                        if arch != "coupling" and (S == 4 or (arch == "affine" and U != 15)):
                            continue  # num_stages (and, for "affine", num_units) do not enter these stacks
                        g.append(row(arch=arch, D=D, U=U, S=S, no_grad=True, **o))
                        if U != 16:
                            g.append(row(arch=arch, D=D, U=U, S=S, p_grad=True, **o))
    for o in ops_:
        for arch, D in (("coupling", 64), ("coupling", 32), ("coupling", 5), ("coupling", 48), ("coupling", 33),
                        ("AR", 5), ("AR", 48)):
            base = dict(arch=arch, D=D, **o)
            for sh in shapes[1:]:  # batch layouts, with and without autograd
                g.append(row(no_grad=True, **base, **sh))
                g.append(row(p_grad=True, **base, **sh))
            for fusion in ("LAYER", "FLOW"):
                g.append(row(fusion=fusion, no_grad=True, **base))
                g.append(row(fusion=fusion, p_grad=True, **base))
            for sup in ("interval", "simplex"):
                g.append(row(sup=sup, no_grad=True, **base))
                g.append(row(sup=sup, p_grad=True, **base))
                g.append(row(sup=sup, fusion="LAYER", no_grad=True, **base))
                g.append(row(sup=sup, override=True, no_grad=True, **base))
            # autograd state: nothing requires grad with grad mode on, z requires grad, both, and both under no_grad
            g.append(row(**base))
            g.append(row(z_grad=True, **base))
            g.append(row(z_grad=True, p_grad=True, **base))
            g.append(row(z_grad=True, p_grad=True, no_grad=True, **base))
            g.append(row(p_grad=True, no_grad=True, **base))
            g.append(row(sup="interval", z_grad=True, **base))
            for sg in (dict(stats_graph=True), dict(stats_graph=True, p_grad=True), dict(stats_graph=True, no_grad=True),
                       dict(stats_graph=True, sup="interval")):
                g.append(row(**base, **sg))
            g.append(row(zdtype="float64", no_grad=True, **base))
            g.append(row(zdtype="float64", p_grad=True, **base))
            for sw in ("fused_batch_forward", "reversible_training", "fused_ar_training"):
                g.append(row(off=sw, no_grad=True, **base))
                g.append(row(off=sw, p_grad=True, **base))
                g.append(row(off=sw, p_grad=True, S=1, **base))
            g.append(row(reduce=True, no_grad=True, **base))
            g.append(row(reduce=True, p_grad=True, **base))
            g.append(row(reduce=True, no_grad=True, M=1, N=1, **base))
            g.append(row(override=True, no_grad=True, **base))
            g.append(row(override=True, p_grad=True, **base))
            g.append(row(override=True, **base))
            if o["op"] != "forward":
                for zdim in (2, 1):
                    g.append(row(zdim=zdim, no_grad=True, **base))
                    g.append(row(zdim=zdim, p_grad=True, **base))
                    g.append(row(zdim=zdim, no_grad=True, rows="M", M=3, **base))
            else:
                for draw in ("torch32", "torch64"):
                    g.append(row(draw=draw, no_grad=True, **base))
                    g.append(row(draw=draw, p_grad=True, **base))
                    g.append(row(draw=draw, fusion="LAYER", no_grad=True, **base))
                    g.append(row(draw=draw, sup="interval", no_grad=True, **base))
                    g.append(row(draw=draw, override=True, no_grad=True, **base))
                    g.append(row(draw=draw, no_grad=True, rows="M", M=3, N=31, **base))
    seen, out = set(), []
    for r in g:
        if row_id(r) not in seen:
            seen.add(row_id(r))
            out.append(r)
    return out


GRID = _grid()


def run_row(r):
    """Build the flow and the inputs the row names, make the call under the recorders, return its trace."""
    D, M, N = r["D"], r["M"], r["N"]
    torch.manual_seed(0)
    sup = {None: lambda: None, "interval": lambda: tnf.ToInterval(D, [-1.0] * D, [2.0] * D),
           "simplex": lambda: tnf.ToSimplex(D)}[r["sup"]]()
    nf = tnf.NormFlow(D, True, r["arch"], r["S"], L, r["U"], support_layer=sup, device="cpu")
    nf.fusion = {"AUTO": _lib.FUSE_AUTO, "LAYER": _lib.FUSE_LAYER, "FLOW": _lib.FUSE_FLOW}[r["fusion"]]
    if r["off"]:
        setattr(nf, r["off"], False)
    if r["reduce"]:
        nf.batch_stats_reduce = lambda moments: moments
    if r["override"]:
        nf._fused_ok = lambda z, p: False
    if r["stats_graph"]:
        for b in nf.bijectors:
            if b.name == "BatchNorm":
                b._last_mean = torch.zeros(D, requires_grad=True)
    params = torch.zeros(M if r["rows"] == "M" else 1, nf.D_params, requires_grad=r["p_grad"])
    D_z = D + 1 if r["sup"] == "simplex" and r["op"] != "forward" else D
    z = torch.zeros((M, N, D_z)[3 - r["zdim"]:], dtype=getattr(torch, r["zdtype"]), requires_grad=r["z_grad"])
    trace = []
    with recording(trace), (torch.no_grad() if r["no_grad"] else torch.enable_grad()):
        try:
            if r["op"] == "log_prob":
                nf.log_prob(z, params)
            elif r["op"] == "inverse":
                nf.inverse_and_log_det(z, params)
            else:
                P = params.size(0)
                omega = {"numpy64": np.zeros((P, N, D)), "torch32": torch.zeros(P, N, D),
                         "torch64": torch.zeros(P, N, D, dtype=torch.float64)}[r["draw"]]
                nf._forward_from(omega, params, r["freeze_bn"])
        except _Reached:
            pass
        except Exception as exc:  # noqa: BLE001 -- the type of any other exception is the trace's last entry
            trace.append("raises " + type(exc).__name__)
    return trace


def family_of(trace):
    last = trace[-1] if trace else ""
    return FAMILY.get(last) or FAMILY.get(last.split("(")[0])


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_grid_is_the_recorded_one():
    assert [row_id(r) for r in GRID] == list(_table()), "the grid and tests/route_table.json list different rows"


@pytest.mark.parametrize("r", GRID, ids=row_id)
def test_route_unchanged(r):
    assert run_row(r) == _table()[row_id(r)]


def test_every_family_has_three_rows():
    count = dict.fromkeys(FAMILIES, 0)
    for trace in _table().values():
        fam = family_of(trace)
        if fam is not None:
            count[fam] += 1
    assert all(n >= 3 for n in count.values()), count


@pytest.mark.parametrize("name", ["_stats_in_graph", "_train_path"])
def test_shared_facts_evaluated_at_most_once_per_call(name, monkeypatch):
    """The statistics walk and the choice of the training pair happen once per public call, not once per family."""
    calls = []
    real = getattr(tnf.NormFlow, name)
    monkeypatch.setattr(tnf.NormFlow, name, lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    for r in GRID:
        del calls[:]
        run_row(r)
        assert len(calls) <= 1, (row_id(r), len(calls))


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_route_table.py --write")
    table = {row_id(r): run_row(r) for r in GRID}
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    fams = [family_of(t) for t in table.values()]
    print(len(table), "rows;", {f: fams.count(f) for f in FAMILIES}, "other:", fams.count(None))
