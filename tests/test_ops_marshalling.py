"""What every wrapper of ops.py / grad.py hands to the C ABI: a fixed grid of calls against tests/ops_marshalling.json.

One level below tests/test_route_table.py.  The harness knows nothing of how the wrappers are written.  It replaces
`_lib.require_device` (the CPU stands in for the device), `_lib.stream_ptr` (0) and the `lib` of _lib.py, ops.py and
grad.py by a recorder: the pure queries (`*_workspace_bytes`, `*_supported`, `*_floats`, `*_num_params`, tnf_ef_num_eta,
tnf_has_fast_path, tnf_get_option, tnf_set_option, tnf_last_error) go to the real library, every other entry is noted
and answers 0 without running.  A row's trace is, per `lib` call, the entry name with every number as it is and every
pointer as
    null       None                          in:<name>  the data_ptr() of a tensor the row passed in (no copy was made)
    ws         inside a buffer of ops._ws_cache         new        anything else: a staged copy or an output
    @<k>       a pointer first seen as the k-th `new` of this trace (the output of one call is the input of the next)
and the integer after a `ws` pointer as `ok` when it lies between the answer of the trace's last workspace query and
the buffer's size.  After the calls the row notes shape, dtype and requires_grad of what came back (values are
uninitialised memory), the gradients, or the type and message of the exception.  Only module attributes are patched,
so this file runs unchanged on any commit: `python tests/test_ops_marshalling.py --write` records the table (done
once, on the commit whose marshalling is to be preserved; the table is not regenerated afterwards).  Needs the built
library for the queries only; no GPU."""
import contextlib
import ctypes
import functools
import inspect
import json
import os
import re
import sys
import threading

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from torch_nf_amd import _lib, grad, ops  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "ops_marshalling.json")
F32, F64 = torch.float32, torch.float64
REAL = _lib.lib
QUERY = re.compile(r"_workspace_bytes$|_supported$|_floats$|_num_params$|^tnf_ef_num_eta$|^tnf_has_fast_path$|"
                   r"^tnf_get_option$|^tnf_set_option$|^tnf_last_error$")
SILENT = ("tnf_get_option", "tnf_last_error")  # how often the options are read is not part of the contract


class _KeepAlive(TorchDispatchMode):
    """Holds every tensor a row creates until the row ends, so that no address is handed out twice within a trace."""

    def __init__(self):
        super().__init__()
        self.kept = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.kept.append(out)
        return out


class Recorder(object):
    """Stands in for `_lib.lib` during one row."""

    def __init__(self, row):
        self.row = row
        self.trace = row.trace
        self.new = []
        self.last_query = 0

    def _pointer(self, p):
        if p is None:
            return "null"
        if p == 0:
            return "0"
        for name, t in self.row.named:
            if t.numel() and t.data_ptr() == p:
                return "in:" + name
        for buf in ops._ws_cache.values():
            if buf.data_ptr() <= p < buf.data_ptr() + buf.numel():
                return "ws"
        if p in self.new:
            return "@%d" % self.new.index(p)
        self.new.append(p)
        return "new"

    def _ws_size(self, v):
        sizes = [buf.numel() for buf in ops._ws_cache.values()]
        return "ok" if sizes and self.last_query <= v <= max(sizes) else repr(v)

    def __getattr__(self, name):
        res, argtypes = _lib.SIGNATURES[name]
        real = getattr(REAL, name)

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            if name in SILENT:
                return real(*args)
            noted, after_ws = [], False
            for a, ty in zip(args, argtypes):
                if ty is ctypes.c_void_p:
                    noted.append(self._pointer(a))
                elif ty is ctypes.c_float:
                    noted.append(repr(float(a)))
                else:
                    assert isinstance(a, int), (name, a)
                    noted.append(self._ws_size(a) if after_ws else repr(int(a)))
                after_ws = noted[-1] == "ws"
            line = "%s(%s)" % (name, ",".join(noted))
            if QUERY.search(name):
                rc = real(*args)
                if name.endswith("_workspace_bytes"):
                    self.last_query = rc
                self.trace.append("%s=%d" % (line, rc))
                return rc
            self.trace.append(line)
            if self.row.poke_flag and name == "tnf_flow_log_prob_bwd_rev_f32" and args[-2] is not None:
                ctypes.c_int32.from_address(args[-2]).value = 1  # the kernel's overflow flag, as the host will read it
            return self.row.answers.get(name, 0)

        return call


def _desc(t):
    if t is None:
        return "None"
    return "%s%s%s" % (str(t.dtype).replace("torch.", ""), list(t.shape), "+grad" if t.requires_grad else "")


class Row(object):
    """What a row function gets: named input tensors, the notes, the backward."""

    def __init__(self):
        self.trace, self.named, self.answers, self.poke_flag = [], [], {}, False

    def t(self, name, shape, dtype=F32, grad=False, kind="c"):
        """A named input.  kind: c contiguous | nc non-contiguous (last two dimensions swapped in memory) | and for
        (M, P) rows: wide (row stride > P) | expand (one row, stride(0) == 0) | inner (inner stride 2)."""
        shape = tuple(shape)
        if kind == "c":
            base, view = shape, lambda b: b
        elif kind == "nc":
            base, view = shape[:-2] + (shape[-1], shape[-2]), lambda b: b.transpose(-1, -2)
        elif kind == "wide":
            base, view = (shape[0], shape[1] + 3), lambda b: b[:, 1:1 + shape[1]]
        elif kind == "expand":
            base, view = (1, shape[1]), lambda b: b.expand(shape)
        else:
            assert kind == "inner", kind
            base, view = (shape[0], 2 * shape[1]), lambda b: b[:, ::2]
        out = view(torch.zeros(base, dtype=dtype, requires_grad=grad))
        self.named.append((name, out))
        return out

    def ret(self, out):
        outs = out if isinstance(out, (tuple, list)) else (out,)
        self.trace.append("-> " + " ".join(_desc(t) for t in outs))
        return outs

    def backward(self, outs, wrt, present=None, thread=False):
        """Gradients g<i> into the outputs listed in `present` (default: all that carry a graph), out of `wrt`."""
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        idx = [i for i in (range(len(outs)) if present is None else present)
               if outs[i] is not None and outs[i].requires_grad]
        wrt = [w for w in wrt if w.requires_grad]
        if not idx or not wrt:
            self.trace.append("no graph")
            return
        gs = [self.t("g%d" % i, outs[i].shape, outs[i].dtype) for i in idx]
        self.trace.append("backward " + ",".join("g%d" % i for i in idx))
        box = []

        def run():
            with _KeepAlive() as keep:
                box.append(keep)
                try:
                    box.append(torch.autograd.grad([outs[i] for i in idx], wrt, gs, allow_unused=True))
                except Exception as exc:  # noqa: BLE001
                    box.append(exc)

        if thread:  # a thread of its own: the library's options are at their defaults there, as on autograd's
            th = threading.Thread(target=run)
            th.start()
            th.join()
        else:
            run()
        self.kept = box[0]
        if isinstance(box[1], Exception):
            raise box[1]
        self.trace.append("grads " + " ".join(_desc(g) for g in box[1]))


@contextlib.contextmanager
def recording(row):
    rec = Recorder(row)
    with pytest.MonkeyPatch.context() as mp, _KeepAlive():
        mp.setattr(_lib, "require_device", lambda: torch.device("cpu"))
        mp.setattr(_lib, "stream_ptr", lambda: 0)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
        for mod in (_lib, ops, grad):  # _lib: the option re-entry of a backward is part of the trace
            mp.setattr(mod, "lib", rec)
        for name in ("check_overflow", "overflow_recovery", "overflow_fallbacks", "last_overflow_flag"):
            mp.setattr(ops._FlowLogProbRevFn, name, getattr(ops._FlowLogProbRevFn, name))  # restored after the row
        ops._ws_cache.clear()
        try:
            yield
        finally:
            ops._ws_cache.clear()


# ---- the grid --------------------------------------------------------------------------------------------------------
ROWS = {}


def add(id_, fn, **kw):
    assert id_ not in ROWS, id_
    ROWS[id_] = functools.partial(fn, **kw)


def _kw_id(kw):
    return " ".join("%s=%s" % (k, str(v).replace("torch.", "")) for k, v in kw.items())


def family(prefix, fn, variants):
    sig = inspect.signature(fn)
    for kw in variants:
        assert set(kw) <= set(sig.parameters), kw
        add((prefix + " " + _kw_id(kw)).strip(), fn, **kw)


D, L, U, P = 4, 2, 3, 24  # the bijector layers; no wrapper looks at the number of parameter columns
M_, N_ = 3, 5
PKINDS = ("c", "wide", "expand", "inner")


def layer(r, entry="coupling", dtype=F32, pdtype=None, pkind="c", zkind="c", Mz=M_, Mp=M_, N=N_, zgrad=True,
          pgrad=True, present=None, inverse=False, zdim=3, Dz=D, mdtype=None, enable_grad=True):
    z = r.t("z", (Mz, N, Dz)[3 - zdim:], dtype, zgrad, zkind)
    p = r.t("params", (Mp, P), pdtype or dtype, pgrad, pkind)
    with (torch.enable_grad() if enable_grad else torch.no_grad()):
        if entry == "coupling":
            out = ops.coupling(z, p, D, L, U, True, inverse)
        elif entry == "affine":
            out = ops.affine(z, p, D, inverse)
        else:
            out = ops.maf(z, p, r.t("masks", (17,), mdtype or dtype), D, L, U, inverse)
    r.backward(r.ret(out), [z, p], present)


LAYER_VARIANTS = ([dict(pkind=k) for k in PKINDS] + [dict(Mp=1), dict(Mp=1, pkind="wide"), dict(Mz=1), dict(zkind="nc"),
                  dict(dtype=F64), dict(dtype=F64, pkind="wide", zkind="nc"), dict(N=0), dict(N=0, enable_grad=False),
                  dict(present=(0,)), dict(present=(1,)), dict(zgrad=False), dict(pgrad=False), dict(inverse=True),
                  dict(enable_grad=False), dict(enable_grad=False, Mp=1, zkind="nc"), dict(enable_grad=False, Mz=1),
                  dict(zdim=2), dict(Dz=D + 1), dict(pdtype=F64), dict(Mz=2), dict(dtype=torch.float16)])
for _e in ("coupling", "affine", "maf"):
    family(_e, functools.partial(layer, entry=_e), LAYER_VARIANTS)
family("maf", functools.partial(layer, entry="maf"), [dict(mdtype=F64), dict(mdtype=F64, enable_grad=False),
                                                       dict(inverse=True, Mz=1), dict(inverse=True, present=(1,))])


def maf_inverse_alpha(r, dtype=F32, mdtype=F32, N=N_):
    r.ret(ops.maf_inverse_alpha_raw(r.t("x", (M_, N, D), dtype), r.t("params", (1, P), dtype), r.t("masks", (17,), mdtype),
                                    D, L, U))


family("maf_inverse_alpha", maf_inverse_alpha, [dict(), dict(dtype=F64), dict(N=0)])


def bn_apply(r, dtype=F32, sdtype=F32, sgrad=False, zgrad=True, inverse=False, zkind="c", present=None, zdim=3):
    z = r.t("z", (M_, N_, D)[3 - zdim:], dtype, zgrad, zkind)
    mean, alpha = r.t("mean", (D,), sdtype, sgrad), r.t("alpha", (D,), sdtype, sgrad)
    r.backward(r.ret(ops.bn_apply(z, mean, alpha, inverse)), [z, mean, alpha], present)


family("bn_apply", bn_apply, [dict(), dict(dtype=F64), dict(sdtype=F64), dict(sgrad=True), dict(sgrad=True, inverse=True),
                              dict(sgrad=True, zgrad=False), dict(zgrad=False), dict(inverse=True), dict(zkind="nc"),
                              dict(present=(0,)), dict(present=(1,)), dict(sgrad=True, present=(1,)), dict(zdim=2),
                              dict(dtype=torch.int32, zgrad=False)])


def _ident(t):
    return t


def bn_batch(r, dtype=F32, zgrad=True, zkind="c", present=None, reduce=False, shape=(M_, N_, D), kernels=False):
    z = r.t("z", shape, dtype, zgrad, zkind)
    if kernels:
        out = ops.bn_batch_forward_sharded(z, 1e-5, _ident, ops.HipBnShardKernels)
    else:
        out = ops.bn_batch_forward(z, 1e-5, _ident if reduce else None)
    r.backward(r.ret(out), [z], present)


family("bn_batch", bn_batch, [dict(reduce=red, **kw) for red in (False, True) for kw in (
    dict(), dict(zgrad=False), dict(zkind="nc"), dict(present=(0,)), dict(present=(1,)), dict(present=(2,)),
    dict(present=(3,)), dict(present=(0, 1)), dict(dtype=F64, zgrad=False), dict(shape=(N_, D), zgrad=False))]
    + [dict(shape=(1, 1, D), zgrad=False), dict(kernels=True), dict(kernels=True, zkind="nc", zgrad=False)])


def base_density(r, dtype=F32, kind="c"):
    r.ret(ops.base_log_density_f64(r.t("omega", (M_, N_, D), dtype, kind=kind)))


family("base_log_density", base_density, [dict(), dict(dtype=F64), dict(kind="nc"), dict(dtype=torch.float16)])

# ---- RealNVP flows (float32) -----------------------------------------------------------------------------------------
FD, FS, FU, FP, FN = 64, 2, 15, 40, 32  # a shape with the whole-flow kernel, the reversible pair and the per-layer pair
FUSE = {"AUTO": _lib.FUSE_AUTO, "LAYER": _lib.FUSE_LAYER, "FLOW": _lib.FUSE_FLOW}


def _stats(r, S, Dn, sdtype=F32, sgrad=False, flat=False):
    shape = (2 * S * Dn,) if flat else (2 * S, Dn)
    return r.t("bn_mean", shape, sdtype, sgrad), r.t("bn_alpha", shape, sdtype, sgrad)


def flow_log_prob(r, padded=False, Dn=FD, U_=FU, pkind="c", zkind="c", Mz=1, Mp=1, N=FN, fusion="AUTO", lp=True, z0=False,
                  sld=False, reruns=False, consts=False, sdtype=F32, sgrad=False, zdtype=F32, zdim=3):
    z = r.t("z", (Mz, N, Dn)[3 - zdim:], zdtype, kind=zkind)
    p = r.t("params", (Mp, FP), kind=pkind)
    mean, alpha = _stats(r, FS, Dn, sdtype, sgrad)
    if padded:
        out = ops.flow_padded_log_prob_raw(z, p, mean, alpha, Dn, FS, L, U_, want_z0=z0, want_sld=sld, want_lp=lp,
                                           count_reruns=reruns)
    else:
        out = ops.flow_log_prob_raw(z, p, mean, alpha, Dn, FS, L, U_, FUSE[fusion], want_z0=z0, want_sld=sld, want_lp=lp,
                                    interval_consts=r.t("consts", (7, Dn)) if consts else None, count_reruns=reruns)
    r.ret(out)


def flow_forward(r, padded=False, Dn=FD, pkind="c", zkind="c", Mz=1, Mp=1, N=FN, fusion="AUTO", log_q=False, consts=False,
                 sdtype=F32, zdtype=F32, eunsupported=False, zdim=3):
    if eunsupported:
        r.answers["tnf_flow_forward_logq_f32"] = _lib.EUNSUPPORTED
    o = r.t("omega", (Mz, N, Dn)[3 - zdim:], zdtype, kind=zkind)
    p = r.t("params", (Mp, FP), kind=pkind)
    mean, alpha = _stats(r, FS, Dn, sdtype)
    if padded:
        out = ops.flow_padded_forward_raw(o, p, mean, alpha, Dn, FS, L, FU, want_log_q=log_q)
    else:
        out = ops.flow_forward_raw(o, p, mean, alpha, Dn, FS, L, FU, FUSE[fusion],
                                   interval_consts=r.t("consts", (7, Dn)) if consts else None, want_log_q=log_q)
    r.ret(out)


_SHAPES = ([dict(pkind=k, Mz=M_, Mp=M_) for k in PKINDS] + [dict(pkind="wide"), dict(Mz=M_), dict(Mp=M_), dict(zkind="nc"),
           dict(N=0), dict(Mz=2, Mp=M_), dict(zdim=2), dict(zdtype=F64), dict(sdtype=F64)])
for _pad, _Dn in ((False, FD), (True, 5)):
    _name = "flow_padded" if _pad else "flow"
    family(_name + "_log_prob", functools.partial(flow_log_prob, padded=_pad, Dn=_Dn),
           _SHAPES + [dict(sgrad=True), dict(z0=True), dict(sld=True), dict(lp=False, z0=True, sld=True), dict(reruns=True),
                      dict(reruns=True, N=0), dict(reruns=True, lp=False, sld=True)])
    family(_name + "_forward", functools.partial(flow_forward, padded=_pad, Dn=_Dn),
           _SHAPES + [dict(log_q=True), dict(log_q=True, N=0), dict(log_q=True, Mp=M_, pkind="wide")])
family("flow_log_prob", flow_log_prob, [dict(fusion="LAYER"), dict(fusion="FLOW"), dict(consts=True),
                                        dict(consts=True, reruns=True), dict(fusion="LAYER", z0=True, Mp=M_),
                                        dict(U_=16), dict(U_=16, fusion="FLOW")])
family("flow_forward", flow_forward, [dict(fusion="LAYER"), dict(fusion="FLOW"), dict(consts=True), dict(consts=True, log_q=True),
                                      dict(fusion="LAYER", log_q=True), dict(fusion="FLOW", log_q=True),
                                      dict(log_q=True, eunsupported=True), dict(log_q=True, eunsupported=True, consts=True)])


def flow_forward_batch(r, pkind="c", zkind="c", M=1, Mp=1, reduce=False, steps=False, pgrad=False):
    o = r.t("omega", (M, FN, FD), kind=zkind)
    p = r.t("params", (Mp, FP), grad=pgrad, kind=pkind)
    if steps:
        out = ops.run_batch_steps(ops.FlowForwardBatchSteps(o, p, FD, FS, L, FU, 1e-5), _ident if reduce else None)
    else:
        out = ops.flow_forward_batch_raw(o, p, FD, FS, L, FU, 1e-5, _ident if reduce else None)
    r.ret(out)


family("flow_forward_batch", flow_forward_batch,
       [dict(), dict(reduce=True), dict(steps=True), dict(steps=True, reduce=True), dict(pgrad=True), dict(zkind="nc"),
        dict(M=M_, Mp=M_, pkind="wide"), dict(M=M_, Mp=M_, pkind="expand", reduce=True), dict(M=M_, Mp=M_, pkind="inner"),
        dict(M=M_), dict(steps=True, M=M_, Mp=M_, pkind="wide")])


def flow_forward_train(r, pkind="c", zkind="c", M=1, Mp=1, ograd=False, pgrad=True, present=None):
    o = r.t("omega", (M, FN, FD), grad=ograd, kind=zkind)
    p = r.t("params", (Mp, FP), grad=pgrad, kind=pkind)
    r.backward(r.ret(ops.flow_forward_train(o, p, FD, FS, L, FU, 1e-5)), [o, p], present)


family("flow_forward_train", flow_forward_train,
       [dict(), dict(ograd=True), dict(present=(0,)), dict(present=(1,)), dict(zkind="nc"), dict(M=M_),
        dict(ograd=True, pgrad=False)] + [dict(M=M_, Mp=M_, pkind=k) for k in PKINDS])


def flow_log_prob_train(r, pkind="c", zkind="c", M=1, Mp=1, N=FN, zgrad=False, pgrad=True, reversible=True, mode=None,
                        check_overflow=True, poke=False, sdtype=F32, S=FS):
    if mode is not None:
        ops._FlowLogProbRevFn.overflow_recovery = mode
    ops._FlowLogProbRevFn.check_overflow = check_overflow
    r.poke_flag = poke
    z = r.t("z", (M, N, FD), grad=zgrad, kind=zkind)
    p = r.t("params", (Mp, FP), grad=pgrad, kind=pkind)
    mean, alpha = _stats(r, S, FD, sdtype)
    out = r.ret(ops.flow_log_prob_train(z, p, mean, alpha, FD, S, L, FU, reversible=reversible))
    r.backward(out, [z, p])
    r.trace.append("fallbacks %d" % ops._FlowLogProbRevFn.overflow_fallbacks)


_TRAIN = ([dict(), dict(zgrad=True), dict(zgrad=True, pgrad=False), dict(zkind="nc"), dict(sdtype=F64), dict(M=M_)]
          + [dict(M=M_, Mp=M_, pkind=k, zgrad=zg) for k in PKINDS for zg in (False, True)])
family("flow_log_prob_train", flow_log_prob_train,
       [dict(reversible=rev, **kw) for rev in (True, False) for kw in _TRAIN]
       + [dict(mode=m, zgrad=zg) for m in ("device", "host", "off") for zg in (False, True)]
       + [dict(check_overflow=False), dict(mode="host", poke=True), dict(mode="host", poke=True, zgrad=True),
          dict(mode="device", poke=True), dict(N=8), dict(N=8, mode="host"), dict(M=M_, Mp=M_, N=8), dict(S=5),
          dict(reversible=False, N=8)])


def flow_options(r, key="force_generic", entry="flow"):
    """An option set around the forward only: the backward, on a thread of its own, must re-enter it."""
    z = r.t("z", (1, FN, FD))
    p = r.t("params", (1, FP), grad=True)
    mean, alpha = _stats(r, FS, FD)
    if key == "force_generic":
        ops.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 1)
        try:
            out = ops.flow_log_prob_train(z, p, mean, alpha, FD, FS, L, FU, reversible=entry == "rev")
        finally:
            ops.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 0)
    else:
        with ops.operand_precision("bf16"):
            r.trace.append("precision " + ops.current_operand_precision())
            out = ops.flow_log_prob_train(z, p, mean, alpha, FD, FS, L, FU, reversible=entry == "rev")
        r.trace.append("precision " + ops.current_operand_precision())
    r.backward(r.ret(out), [p], thread=True)


family("options", flow_options, [dict(key=k, entry=e) for k in ("force_generic", "bf16") for e in ("rev", "layers")])


def options_layer(r, entry="coupling"):
    ops.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 1)
    try:
        z, p = r.t("z", (1, N_, D), grad=True), r.t("params", (1, P), grad=True)
        if entry == "coupling":
            out = ops.coupling(z, p, D, L, U, True, False)
        else:
            with ops.operand_precision("bf16"):
                out = ops.maf(z, p, r.t("masks", (17,)), D, L, U, True)
    finally:
        ops.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 0)
    r.backward(r.ret(out), [z, p], thread=True)


family("options_layer", options_layer, [dict(entry="coupling"), dict(entry="maf")])


def predicates(r):
    r.trace.append("has_fast_path %s %s" % (ops.has_fast_path(FD, L, FU), ops.has_fast_path(5, L, 40)))
    r.trace.append("resolve_fusion %s %s" % (ops.resolve_fusion(FD, FS, L, FU, _lib.FUSE_AUTO),
                                             ops.resolve_fusion(5, FS, L, FU, _lib.FUSE_AUTO)))
    r.trace.append("padded %s %s" % (ops.flow_padded_supported(5, FS, L, FU), ops.flow_padded_supported(32, FS, L, FU)))
    r.trace.append("train %s %s" % (ops.flow_train_supported(1, 1, FN, FD, FS, L, FU),
                                    ops.flow_train_supported(2, 3, FN, FD, FS, L, FU)))
    r.trace.append("rev %s %s" % (ops.flow_train_rev_supported(1, 1, FN, FD, FS, L, FU),
                                  ops.flow_train_rev_supported(M_, M_, 8, FD, FS, L, FU)))
    r.trace.append("cond %s %s" % (ops.cond_flow_supported(FD, FS, L, FU, 50), ops.cond_flow_supported(FD, FS, L, FU, 200)))
    r.trace.append("ar %s %s" % (ops.ar_flow_supported(5, L, FU), ops.ar_flow_train_supported(2, 3, 5, L, FU)))
    r.trace.append("ar_train %s" % ops.ar_flow_train_supported(1, 1, 5, L, FU))
    r.trace.append("ef_num_eta %d" % ops.ef_num_eta(_lib.EF_MVN, D))
    ops.ef_num_eta(7, D)


add("predicates", predicates)

# ---- support layers, exponential families ----------------------------------------------------------------------------


def to_interval(r, dtype=F32, cdtype=F32, zgrad=True, zkind="c", inverse=False, present=None, Dc=D, zdim=3):
    z = r.t("z", (M_, N_, D)[3 - zdim:], dtype, zgrad, zkind)
    r.backward(r.ret(ops.to_interval(z, r.t("consts", (7, Dc), cdtype), inverse)), [z], present)


def to_simplex(r, dtype=F32, zgrad=True, zkind="c", present=None, zdim=3):
    z = r.t("z", (M_, N_, D)[3 - zdim:], dtype, zgrad, zkind)
    r.backward(r.ret(ops.to_simplex(z, D + 1)), [z], present)


_SUP = [dict(), dict(dtype=F64), dict(zgrad=False), dict(zkind="nc"), dict(present=(0,)), dict(present=(1,)), dict(zdim=2)]
family("to_interval", to_interval, _SUP + [dict(cdtype=F64), dict(inverse=True), dict(Dc=D + 1)])
family("to_simplex", to_simplex, _SUP)


def ef_suffstats(r, dtype=F32, fam=_lib.EF_MVN, zgrad=True, zkind="c", zdim=3):
    z = r.t("z", (M_, N_, D)[3 - zdim:], dtype, zgrad, zkind)
    r.backward(r.ret(ops.ef_suffstats(z, fam)), [z])


def ef_dot(r, dtype=F32, edtype=None, fam=_lib.EF_MVN, zgrad=True, egrad=True, zkind="c", ekind="c", Me=M_, cols=None,
           zdim=3):
    z = r.t("z", (M_, N_, D)[3 - zdim:], dtype, zgrad, zkind)
    eta = r.t("eta", (Me, cols or REAL.tnf_ef_num_eta(fam, D)), edtype or dtype, egrad, ekind)
    r.backward(r.ret(ops.ef_dot(z, eta, fam)), [z, eta])


family("ef_suffstats", ef_suffstats, [dict(), dict(dtype=F64), dict(fam=_lib.EF_DIRICHLET), dict(zgrad=False),
                                      dict(zkind="nc"), dict(zdim=2), dict(fam=7, zgrad=False)])
family("ef_dot", ef_dot, [dict(), dict(dtype=F64), dict(fam=_lib.EF_DIRICHLET), dict(zgrad=False), dict(egrad=False),
                          dict(zgrad=False, egrad=False), dict(zkind="nc"), dict(ekind="wide"), dict(ekind="inner"),
                          dict(Me=2), dict(cols=3), dict(edtype=F64), dict(zdim=2)])

# ---- conditional flow, AR flow ---------------------------------------------------------------------------------------
CP = 30


def cond_flow(r, entry="log_prob", H=50, M=M_, z0=False, sld=False, sdtype=F32, hkind="c", zdtype=F32, zgrad=False,
              wgrad=True, hgrad=True, Dz=FD):
    z = r.t("z", (M, Dz), zdtype, zgrad)
    h = r.t("h", (M, H), grad=hgrad and entry == "train", kind=hkind)
    w = r.t("weight", (CP, H), grad=wgrad and entry == "train")
    b = r.t("bias", (CP,), grad=wgrad and entry == "train")
    mean, alpha = _stats(r, FS, FD, sdtype)
    if entry == "log_prob":
        r.ret(ops.cond_flow_log_prob_raw(z, h, w, b, mean, alpha, FD, FS, L, FU, want_z0=z0, want_sld=sld))
    elif entry == "forward":
        r.ret(ops.cond_flow_forward_raw(z, h, w, b, mean, alpha, FD, FS, L, FU))
    else:
        r.backward(r.ret(ops.cond_flow_log_prob_train(z, h, w, b, mean, alpha, FD, FS, L, FU)), [z, h, w, b])


family("cond_flow", cond_flow,
       [dict(entry=e, **kw) for e in ("log_prob", "forward", "train")
        for kw in (dict(), dict(H=64), dict(H=20), dict(M=0), dict(sdtype=F64), dict(hkind="wide"), dict(zdtype=F64))]
       + [dict(z0=True), dict(sld=True), dict(z0=True, sld=True), dict(H=200), dict(entry="forward", H=200), dict(Dz=5),
          dict(entry="forward", Dz=5), dict(entry="train", zgrad=True), dict(entry="train", wgrad=False),
          dict(entry="train", hgrad=False, zgrad=True)])
AD = 5


def ar_flow(r, entry="log_prob", pkind="c", zkind="c", Mz=1, Mp=1, N=N_, mdtype=F32, sdtype=F32, lp=True, z0=False, sld=False,
            consts=False, flat=False, pgrad=True, Dz=AD, zdim=3):
    z = r.t("z", (Mz, N, Dz)[3 - zdim:], kind=zkind)
    p = r.t("params", (Mp, P), grad=pgrad and entry == "train", kind=pkind)
    masks = r.t("masks", (17,), mdtype)
    mean, alpha = _stats(r, 1, AD // 1, sdtype, flat=flat)
    c = r.t("consts", (7, AD)) if consts else None
    if entry == "log_prob":
        r.ret(ops.ar_flow_log_prob_raw(z, p, masks, mean, alpha, AD, L, FU, want_lp=lp, want_z0=z0, want_sld=sld,
                                       interval_consts=c))
    elif entry == "forward":
        r.ret(ops.ar_flow_forward_raw(z, p, masks, mean, alpha, AD, L, FU, interval_consts=c))
    else:
        r.backward(r.ret(ops.ar_flow_log_prob_train(z, p, masks, mean, alpha, c, AD, L, FU)), [p])


family("ar_flow", ar_flow,
       [dict(entry=e, **kw) for e in ("log_prob", "forward", "train")
        for kw in ([dict(), dict(consts=True), dict(mdtype=F64), dict(sdtype=F64), dict(flat=True), dict(zkind="nc"),
                    dict(Mz=M_), dict(Mz=2, Mp=M_), dict(Dz=AD + 1), dict(zdim=2)]
                   + [dict(Mz=M_, Mp=M_, pkind=k) for k in PKINDS])]
       + [dict(lp=False, z0=True), dict(sld=True), dict(z0=True, sld=True, consts=True), dict(entry="train", pgrad=False)])


def run_row(id_):
    row = Row()
    with recording(row):
        try:
            ROWS[id_](row)
        except Exception as exc:  # noqa: BLE001 -- type and message of the exception end the trace
            row.trace.append("raises %s: %s" % (type(exc).__name__, exc))
    return row.trace


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_grid_is_the_recorded_one():
    assert list(ROWS) == list(_table()), "the grid and tests/ops_marshalling.json list different rows"


@pytest.mark.parametrize("id_", list(ROWS))
def test_marshalling_unchanged(id_):
    trace = run_row(id_)
    assert trace, "an empty trace pins nothing"
    assert trace == _table()[id_]


def test_every_entry_has_a_row():
    """Every `lib.tnf_*` call in the source text of ops.py and grad.py occurs in the table: a new entry needs a row."""
    called = set()
    for mod in (ops, grad):
        called |= set(re.findall(r"\blib\.(tnf_\w+)\(", inspect.getsource(mod)))
    assert called and called <= set(_lib.SIGNATURES), sorted(called - set(_lib.SIGNATURES))
    seen = set()
    for trace in _table().values():
        seen |= set(line.split("(")[0] for line in trace if line.startswith("tnf_"))
    assert not called - seen, sorted(called - seen)


def test_no_row_is_empty():
    assert all(_table().values())


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_ops_marshalling.py --write")
    table = {id_: run_row(id_) for id_ in ROWS}
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(len(table), "rows;", sum(len(t) for t in table.values()), "lines;",
          sum(1 for t in table.values() if t[-1].startswith("raises")), "raise")
