"""What the wrappers of the seven one-launch coupling families hand to the C ABI: a fixed grid of calls against
tests/family_marshalling.json, by the method of tests/test_ops_marshalling.py (whose rows, pointer vocabulary and notes
these are: see its docstring).

The families: ctxflow_ops, ctxtrain_ops, ctxsample_ops, ctxwide_ops, ctxwidesample_ops, wideflow_ops, widestream_ops.
They hold four bodies -- `*_log_prob_raw`, `*_forward_raw`, the log_prob training pair (`*_log_prob_bwd_raw`,
`*_log_prob_train`) and the sampling training pair (`*_sample_bwd_raw`, `*_sample_train`) -- so one row function serves
each body and is applied to every family that has it.

The recorder differs from that file's in two ways.  An entry's (restype, argtypes) is looked up in every module-level
table of _lib.py whose keys start with `tnf_`, not in SIGNATURES alone; and the recorder replaces the attribute `lib` of
every loaded `torch_nf_amd.*` module that has one whose value is `_lib.lib`, found by scanning sys.modules -- so this file
runs unchanged whatever module a wrapper's body lives in.  The queries (`*_supported`, `*_num_params`, `*_lds_bytes`,
`*_tiles`, `*_waves`, `*_launch_count`, the options) go to the real library; the setters `*_set_tiles` / `*_set_waves`
and every `*_f32` entry are noted and answer 0 without running.  `python tests/test_family_marshalling.py --write`
records the table (done once, on the commit whose marshalling is to be preserved; the table is not regenerated
afterwards).  Needs the built library for the queries only; no GPU."""
import contextlib
import ctypes
import functools
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_ops_marshalling import F32, F64, PKINDS, REAL, Recorder, Row, _KeepAlive, _kw_id  # noqa: E402

from torch_nf_amd import (_lib, ctxflow_ops, ctxsample_ops, ctxtrain_ops, ctxwide_ops, ctxwidesample_ops, ops,  # noqa: E402
                          wideflow_ops, widestream_ops)

TABLE = os.path.join(ROOT, "tests", "family_marshalling.json")
QUERY = re.compile(r"_supported$|_num_params$|_lds_bytes$|(?<!_set)_tiles$|(?<!_set)_waves$|_launch_count$|"
                   r"^tnf_get_option$|^tnf_set_option$|^tnf_last_error$")
SILENT = ("tnf_get_option", "tnf_last_error")  # how often the options are read is not part of the contract


def _signatures():
    """Every entry of every module-level table of _lib.py whose keys start with `tnf_`."""
    out = {}
    for value in vars(_lib).values():
        if isinstance(value, dict) and value and all(isinstance(k, str) and k.startswith("tnf_") for k in value):
            out.update(value)
    return out


SIGNATURES = _signatures()


class FamilyRecorder(Recorder):
    """Stands in for `_lib.lib` during one row: test_ops_marshalling.Recorder's pointers, every table's signatures."""

    def __getattr__(self, name):
        _, argtypes = SIGNATURES[name]
        real = getattr(REAL, name)

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            if name in SILENT:
                return real(*args)
            noted = []
            for a, ty in zip(args, argtypes):
                if ty is ctypes.c_void_p:
                    noted.append(self._pointer(a))
                else:
                    assert isinstance(a, int), (name, a)
                    noted.append(repr(int(a)))
            line = "%s(%s)" % (name, ",".join(noted))
            if QUERY.search(name):
                rc = real(*args)
                self.trace.append("%s=%d" % (line, rc))
                return rc
            self.trace.append(line)
            return 0

        return call


def _lib_holders():
    """The loaded modules of the package whose `lib` is the library itself."""
    return [mod for name, mod in sorted(sys.modules.items())
            if name.startswith("torch_nf_amd.") and mod is not None and vars(mod).get("lib") is REAL]


@contextlib.contextmanager
def recording(row):
    rec = FamilyRecorder(row)
    holders = _lib_holders()
    assert _lib in holders and ops in holders and len(holders) >= 9, [m.__name__ for m in holders]
    with pytest.MonkeyPatch.context() as mp, _KeepAlive():
        mp.setattr(_lib, "require_device", lambda: torch.device("cpu"))
        mp.setattr(_lib, "stream_ptr", lambda: 0)
        for mod in holders:  # _lib too: the option re-entry of a backward is part of the trace
            mp.setattr(mod, "lib", rec)
        yield


# ---- the grid --------------------------------------------------------------------------------------------------------
ROWS = {}
M_, N_, D, S, L = 3, 5, 4, 1, 2  # the smallest shapes that tell the cases apart; no kernel runs
U_NARROW, U_WIDE = 3, 20


def family(fn, targets, variants):
    """One row function, applied to every family that has its body: targets are (module, attribute, U, more keywords)."""
    for mod, attr, U, more in targets:
        for kw in variants + more:
            id_ = ("%s.%s %s" % (mod.__name__.rsplit(".", 1)[1], attr, _kw_id(kw))).strip()
            assert id_ not in ROWS, id_
            ROWS[id_] = functools.partial(fn, mod=mod, attr=attr, U=U, **kw)


def _inputs(r, zname, U, Mz=M_, Mp=M_, N=N_, Dz=D, pkind="c", zkind="c", zdtype=F32, pdtype=F32, sdtype=F32, extra=0,
            zgrad=False, pgrad=False):
    """(z or omega, params, bn_mean, bn_alpha); `extra` trailing parameter columns beyond tnf_flow_num_params."""
    P = REAL.tnf_flow_num_params(D, S, L, U)
    assert P > 0, (D, S, L, U)
    z = r.t(zname, (Mz, N, Dz), zdtype, zgrad, zkind)
    p = r.t("params", (Mp, P + extra), pdtype, pgrad, pkind)
    return z, p, r.t("bn_mean", (2 * S, D), sdtype), r.t("bn_alpha", (2 * S, D), sdtype), P


def log_prob_raw(r, mod, attr, U, lp=True, z0=False, sld=False, **kw):
    z, p, mean, alpha, _ = _inputs(r, "z", U, **kw)
    r.ret(getattr(mod, attr)(z, p, mean, alpha, D, S, L, U, want_lp=lp, want_z0=z0, want_sld=sld))


def forward_raw(r, mod, attr, U, **kw):
    o, p, mean, alpha, _ = _inputs(r, "omega", U, **kw)
    r.ret(getattr(mod, attr)(o, p, mean, alpha, D, S, L, U))


_KINDS = [dict(pkind=k) for k in PKINDS]
_COMMON = _KINDS + [dict(zkind="nc"), dict(N=0), dict(Dz=D + 1), dict(zdtype=F64), dict(pdtype=F64), dict(sdtype=F64)]
family(log_prob_raw,
       [(ctxflow_ops, "ctx_flow_log_prob_raw", U_NARROW, []), (ctxwide_ops, "ctx_wide_log_prob_raw", U_WIDE, []),
        (wideflow_ops, "wide_flow_log_prob_raw", U_WIDE, [dict(Mp=1), dict(Mp=1, pkind="wide")]),
        (widestream_ops, "wide_flow_stream_log_prob_raw", U_WIDE, [dict(Mp=1), dict(Mp=1, pkind="wide")])],
       _COMMON + [dict(Mz=1), dict(Mz=2), dict(lp=True), dict(lp=False, z0=True), dict(lp=False, sld=True),
                  dict(lp=True, z0=True, sld=True), dict(lp=False)])
family(forward_raw,
       [(ctxflow_ops, "ctx_flow_forward_raw", U_NARROW, [dict(Mp=1)]), (ctxwide_ops, "ctx_wide_forward_raw", U_WIDE, [dict(Mp=1)]),
        (wideflow_ops, "wide_flow_forward_raw", U_WIDE, [dict(Mp=1), dict(Mp=1, pkind="wide")]),
        (widestream_ops, "wide_flow_stream_forward_raw", U_WIDE, [dict(Mp=1), dict(Mp=1, pkind="wide")])],
       _COMMON + [dict(Mz=1), dict(Mz=2)])


def _zero(t):
    return "None" if t is None else str(bool((t == 0).all()))


def log_prob_bwd_raw(r, mod, attr, U, want_gz=True, gshape=None, gdtype=F32, trailing=False, **kw):
    z0, p, mean, alpha, P = _inputs(r, "z0", U, extra=3 if trailing else 0, **kw)
    g = r.t("g_lp", gshape or tuple(z0.shape[:2]), gdtype)
    gp, gz = r.ret(getattr(mod, attr)(z0, p, mean, alpha, g, D, S, L, U, want_gz=want_gz))
    if trailing or z0.shape[1] == 0:  # `empty` against `zeros` is otherwise invisible to a pointer trace
        r.trace.append("g_params zero: trailing columns %s, all %s" % (_zero(gp[:, P:]), _zero(gp)))


def sample_bwd_raw(r, mod, attr, U, want_go=True, g_z=True, g_sld=True, gzshape=None, gsshape=None, gdtype=F32,
                   trailing=False, **kw):
    z, p, mean, alpha, P = _inputs(r, "z", U, extra=3 if trailing else 0, **kw)
    gz = r.t("g_z", gzshape or tuple(z.shape), gdtype) if g_z else None
    gs = r.t("g_sld", gsshape or tuple(z.shape[:2]), gdtype) if g_sld else None
    gp, go = r.ret(getattr(mod, attr)(z, p, mean, alpha, gz, gs, D, S, L, U, want_go=want_go))
    if trailing or z.shape[1] == 0:
        r.trace.append("g_params zero: trailing columns %s, all %s" % (_zero(gp[:, P:]), _zero(gp)))


_BWD = _KINDS + [dict(), dict(zkind="nc"), dict(N=0), dict(Dz=D + 1), dict(zdtype=F64), dict(pdtype=F64), dict(sdtype=F64),
                 dict(gdtype=F64), dict(Mp=1), dict(Mz=1), dict(trailing=True), dict(trailing=True, N=0),
                 dict(trailing=True, pkind="wide")]
family(log_prob_bwd_raw,
       [(ctxtrain_ops, "ctx_flow_log_prob_bwd_raw", U_NARROW, []), (ctxwide_ops, "ctx_wide_log_prob_bwd_raw", U_WIDE, [])],
       _BWD + [dict(want_gz=False), dict(want_gz=False, trailing=True), dict(want_gz=False, N=0), dict(gshape=(M_, N_ + 1)),
               dict(gshape=(N_, M_)), dict(gshape=(M_, N_, 1))])
family(sample_bwd_raw,
       [(ctxsample_ops, "ctx_flow_sample_bwd_raw", U_NARROW, []),
        (ctxwidesample_ops, "ctx_wide_sample_bwd_raw", U_WIDE, [])],
       _BWD + [dict(want_go=False), dict(want_go=False, trailing=True), dict(want_go=False, N=0), dict(g_sld=False),
               dict(g_z=False), dict(g_z=False, g_sld=False), dict(g_z=False, g_sld=False, zdtype=F64),
               dict(g_sld=False, want_go=False), dict(g_z=False, trailing=True), dict(gzshape=(M_, N_, D + 1)),
               dict(gzshape=(M_, N_)), dict(gsshape=(M_, N_ + 1)), dict(g_z=False, gsshape=(N_, M_)),
               dict(g_sld=False, gdtype=F64)])


def train(r, mod, attr, U, zname="z", present=None, thread=False, enable_grad=True, **kw):
    """A `*_train` autograd entry and its backward.  thread: an option set around the forward only, the backward on a
    thread of its own, which must re-enter it."""
    z, p, mean, alpha, _ = _inputs(r, zname, U, **kw)
    if thread:
        _lib.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 1)
    try:
        with (torch.enable_grad() if enable_grad else torch.no_grad()):
            out = getattr(mod, attr)(z, p, mean, alpha, D, S, L, U)
    finally:
        if thread:
            _lib.lib.tnf_set_option(_lib.OPT_FORCE_GENERIC, 0)
    r.backward(r.ret(out), [z, p], present, thread=thread)


_TRAIN = [dict(pgrad=True), dict(zgrad=True), dict(zgrad=True, pgrad=True), dict(), dict(pgrad=True, enable_grad=False),
          dict(Mz=1, pgrad=True), dict(Mz=1, zgrad=True, pgrad=True), dict(Mz=1, zgrad=True), dict(Mp=1, pgrad=True),
          dict(N=0, pgrad=True), dict(N=0, zgrad=True, pgrad=True), dict(pgrad=True, thread=True),
          dict(zgrad=True, pgrad=True, thread=True), dict(Dz=D + 1, pgrad=True), dict(zdtype=F64, pgrad=True),
          dict(pdtype=F64, pgrad=True), dict(sdtype=F64, pgrad=True), dict(zkind="nc", zgrad=True, pgrad=True)] \
    + [dict(pkind=k, pgrad=True) for k in PKINDS[1:]] + [dict(pkind="wide", zgrad=True, pgrad=True)]
family(train,
       [(ctxtrain_ops, "ctx_flow_log_prob_train", U_NARROW, []), (ctxwide_ops, "ctx_wide_log_prob_train", U_WIDE, [])],
       _TRAIN)
family(functools.partial(train, zname="omega"),
       [(ctxsample_ops, "ctx_flow_sample_train", U_NARROW, []), (ctxwidesample_ops, "ctx_wide_sample_train", U_WIDE, [])],
       _TRAIN + [dict(pgrad=True, present=(0,)), dict(pgrad=True, present=(1,)), dict(pgrad=True, present=(0, 1)),
                 dict(zgrad=True, present=(0,)), dict(zgrad=True, pgrad=True, present=(1,)),
                 dict(pgrad=True, present=(1,), thread=True), dict(N=0, pgrad=True, present=(1,))])


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
    assert list(ROWS) == list(_table()), "the grid and tests/family_marshalling.json list different rows"


@pytest.mark.parametrize("id_", list(ROWS))
def test_marshalling_unchanged(id_):
    trace = run_row(id_)
    assert trace, "an empty trace pins nothing"
    assert trace == _table()[id_]


def test_every_entry_has_a_row():
    """Every `*_f32` entry of the seven families' tables occurs in the table: a new entry needs a row."""
    entries = set()
    for table in (_lib.CTXFLOW_SIGNATURES, _lib.CTXTRAIN_SIGNATURES, _lib.CTXSAMPLE_SIGNATURES, _lib.WIDEFLOW_SIGNATURES,
                  _lib.CTXWIDE_SIGNATURES, _lib.CTXWIDESAMPLE_ENTRIES, _lib.WIDESTREAM_ENTRIES):
        entries |= set(name for name in table if name.endswith("_f32"))
    assert len(entries) == 12, sorted(entries)
    seen = set()
    for trace in _table().values():
        seen |= set(line.split("(")[0] for line in trace if line.startswith("tnf_"))
    assert not entries - seen, sorted(entries - seen)


def test_no_row_is_empty():
    assert all(_table().values())


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_family_marshalling.py --write")
    table = {id_: run_row(id_) for id_ in ROWS}
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=0)
        f.write("\n")
    print(len(table), "rows;", sum(len(t) for t in table.values()), "lines;",
          sum(1 for t in table.values() if t[-1].startswith("raises")), "raise")
