"""Host-side answers of the C ABI, pinned: every call of tests/cabi_host_table.json returns what it returned when
the table was written.

The table was written once, by `python tests/test_cabi_host_table.py --write` on commit d78043d with only this file
added, and is not regenerated afterwards: it is the record of what the argument checks, the size formulas and the
support predicates of torch_nf_amd/csrc/api.hip answered before that file was reorganised.  A rejection or an empty
call is stored under its entry's name as the positional arguments, optionally the tnf_set_option values it runs
under (restored after the row), the return value and, for a negative return, the full message.  The query calls
are the fixed grid of query_grid() below: the table keeps their return values in that order and, per entry, the
message of the first row of each failing code (the other failing rows echo other numbers through the same fail(
site, which also has its row among the rejections).  Pointers are fake addresses that are never dereferenced
(4096 * position, `+2`/`+4`/`+8`/`+16` for a misaligned one, null for NULL): every row either fails an argument
check or returns before the first HIP runtime call.  The return value is compared exactly, a message as (text
before the first ':', the integers in the rest), so two entries may come to word the same fault alike while the
name a message starts with and every number it prints stay.

Three groups of rows:
  query   every *_supported, *_num_params, *_workspace_bytes, *_floats, tnf_ef_num_eta, tnf_has_fast_path over
          D in {2, 5, 8, 31, 32, 33, 63, 64, 128} x L in {1, 2, 3, 5} x U in {15, 16, 17, 64} x S in {1, 4, 7}
          (H in {32, 64, 128, 50} at S = 4 for the conditional flow); the sized ones at (M, N) = (3, 17) on the
          whole grid and at M in {1, 3} x N in {0, 17, 1500} x M_p in {1, M} on its L = 2 part, both `fusion`
          values for tnf_flow_workspace_bytes
  reject  one row per reachable fail( site of the parent's api.hip and entry that reaches it, one fault each --
          the kernel-selection refusals included (bf16 operands without a range kernel, a support layer or log_q
          on a route that has none, TNF_FUSE_FLOW above the LDS limit, an unknown fusion); rows named "order"
          carry two faults and pin which one is reported
  empty   N, M or rows = 0 where the parent returns before touching the runtime, once with valid pointers and
          once with a NULL one (tnf_coupling refuses that one, tnf_to_interval accepts it)

fail( sites of the parent's api.hip (by line) without a row, and why:
  40         check_launch: needs a failed launch
  342, 613   the message prints a pointer with %p (the text is not a function of the arguments alone)
  736, 1166  follow a failed hipMemsetAsync
  863        tnf_ef_dot_backward "no g_eta kernel": ef_dot_bwd_workspace is negative only for a family or D that
             ef_check has refused two lines earlier
Entries without a row: tnf_version, tnf_last_error, tnf_set_launch_gate (they check nothing); tnf_gated_copy_f32,
tnf_diag_launch_count and tnf_ef_launch_count have their rejections only.  Left out as empty calls because the
parent reaches a launcher or the runtime: tnf_cond_flow_log_prob_bwd_f32 with M = 0 (hipMemsetAsync), tnf_affine*,
tnf_bn_*, tnf_ef_*, tnf_base_log_density_f64, the batch-statistics chains and the tnf_flow_forward_train pair.

Needs the built library; no GPU."""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from torch_nf_amd import _lib  # noqa: E402

lib = _lib.lib
TABLE = os.path.join(ROOT, "tests", "cabi_host_table.json")
NO_ROWS = {"tnf_version", "tnf_last_error", "tnf_set_launch_gate"}


def _table():
    with open(TABLE) as f:
        return json.load(f)


def _get_option(key):
    v = ctypes.c_int32(0)
    assert lib.tnf_get_option(key, ctypes.addressof(v)) == 0
    return v.value


def call(entry, args, opts=None):
    """One call under the row's options: (return value, message or None)."""
    before = {int(k): _get_option(int(k)) for k in (opts or {})}
    try:
        for k, v in (opts or {}).items():
            assert lib.tnf_set_option(int(k), v) == 0
        rc = getattr(lib, entry)(*args)
        msg = lib.tnf_last_error().decode() if rc < 0 else None
    finally:
        for k, v in before.items():
            lib.tnf_set_option(k, v)
    return rc, msg


def msg_key(msg):
    head, _, rest = msg.partition(":")
    return head, re.findall(r"-?\d+", rest)


def query_grid():
    """The query calls, in the order their answers are stored: [(entry, args), ...]."""
    out = []

    def q(entry, args):
        out.append((entry, list(args)))

    Ds, Ls, Us, Ss = (2, 5, 8, 31, 32, 33, 63, 64, 128), (1, 2, 3, 5), (15, 16, 17, 64), (1, 4, 7)
    MN = [(M, N) for M in (1, 3) for N in (0, 17, 1500)]
    for D in Ds:
        q("tnf_bn_batch_workspace_bytes", [D])
        for Mp in (1, 3):
            q("tnf_ar_flow_workspace_bytes", [Mp, D])
            q("tnf_ar_flow_bwd_workspace_bytes", [Mp, D])
        for fam in (_lib.EF_MVN, _lib.EF_DIRICHLET):
            q("tnf_ef_num_eta", [fam, D])
            q("tnf_ef_dot_supported", [fam, D])
            for M, N in MN:
                q("tnf_ef_dot_bwd_workspace_bytes", [fam, M, N, D])
        for L in Ls:
            for S in Ss:
                q("tnf_flow_forward_batch_workspace_bytes", [3, D, S, L])
                q("tnf_flow_forward_train_workspace_bytes", [3, 3, 17, D, S, L])
                q("tnf_cond_flow_acts_floats", [17, D, S, L])
                q("tnf_cond_flow_deltas_floats", [17, D, S, L, 64])
                if L == 2:
                    for M, N in MN:
                        for Mp in sorted({1, M}):
                            q("tnf_flow_forward_train_workspace_bytes", [M, Mp, N, D, S, L])
                        q("tnf_flow_forward_batch_workspace_bytes", [M, D, S, L])
            for U in Us:
                for name in ("tnf_has_fast_path", "tnf_ar_flow_supported", "tnf_ar_flow_train_supported", "tnf_maf_num_params"):
                    q(name, [D, L, U])
                for up in (0, 1):
                    q("tnf_coupling_num_params", [D, L, U, up])
                q("tnf_coupling_backward_workspace_bytes", [0, 3, 3, 17, D, L, U, 1])
                q("tnf_maf_backward_workspace_bytes", [0, 3, 3, 17, D, L, U])
                if L == 2:
                    for M, N in MN:
                        for Mp in sorted({1, M}):
                            for dt in (0, 1):
                                q("tnf_coupling_backward_workspace_bytes", [dt, M, Mp, N, D, L, U, 0])
                                q("tnf_maf_backward_workspace_bytes", [dt, M, Mp, N, D, L, U])
                for H in (32, 64, 128, 50):
                    for name in ("tnf_cond_flow_supported", "tnf_cond_flow_workspace_bytes", "tnf_cond_flow_bwd_workspace_bytes"):
                        q(name, [D, 4, L, U, H])
                for S in Ss:
                    for name in ("tnf_flow_num_params", "tnf_flow_fused_supported", "tnf_flow_fused2_supported",
                                 "tnf_flow_fused3_supported", "tnf_flow_train_rev_supported", "tnf_flow_padded_supported"):
                        q(name, [D, S, L, U])
                    q("tnf_cond_flow_supported", [D, S, L, U, 64])
                    sized = [(3, 17)] + (MN if L == 2 else [])
                    for M, N in sized:
                        for fusion in (_lib.FUSE_LAYER, _lib.FUSE_FLOW):
                            q("tnf_flow_workspace_bytes", [M, N, D, S, L, U, fusion])
                        q("tnf_flow_padded_workspace_bytes", [M, N, D, S, L, U])
                        for Mp in sorted({1, M}):
                            q("tnf_flow_train_workspace_bytes", [M, Mp, N, D, S, L, U])
                            q("tnf_flow_train_rev_workspace_bytes", [M, Mp, N, D, S, L, U])
    return out


TABLE_ROWS = _table() if os.path.exists(TABLE) else {"query": {}, "query_msg": {}, "reject": {}, "empty": {}}
GRID = {}
for _entry, _args in query_grid():
    GRID.setdefault(_entry, []).append(_args)


@pytest.mark.parametrize("entry", sorted(TABLE_ROWS["query"]))
def test_queries_unchanged(entry):
    answers, messages = TABLE_ROWS["query"][entry], dict(TABLE_ROWS["query_msg"].get(entry, []))
    assert len(answers) == len(GRID[entry])
    for i, (args, want) in enumerate(zip(GRID[entry], answers)):
        rc, got = call(entry, args)
        assert rc == want, (entry, args, rc, want)
        if i in messages:
            assert msg_key(got) == msg_key(messages[i]), (entry, args, got, messages[i])


def _rows(kind):
    return [dict(r, entry=entry) for entry, rows in TABLE_ROWS[kind].items() for r in rows]


@pytest.mark.parametrize("kind", ["reject", "empty"])
def test_checks_unchanged(kind):
    assert TABLE_ROWS[kind]
    for r in _rows(kind):
        rc, got = call(r["entry"], r["args"], r.get("opts"))
        assert rc == r["rc"], (r, rc, got)
        if r["rc"] < 0:
            assert msg_key(got) == msg_key(r["msg"]), (r, got)
        else:
            assert kind == "empty" or r["entry"] in ("tnf_set_option", "tnf_get_option")


def test_every_entry_has_a_row():
    seen = set(TABLE_ROWS["query"]) | set(TABLE_ROWS["reject"]) | set(TABLE_ROWS["empty"])
    assert set(_lib.SIGNATURES) - seen == NO_ROWS
    only_rejections = {"tnf_gated_copy_f32", "tnf_diag_launch_count", "tnf_ef_launch_count"}
    for name in only_rejections:
        assert name not in TABLE_ROWS["query"] and name not in TABLE_ROWS["empty"]
        assert all(r["rc"] < 0 for r in TABLE_ROWS["reject"][name])


# ---- writing the table (once, on the parent) ---------------------------------------------------------------------------
def _prototypes():
    """entry -> parameter names of include/tnf.h, under the short names api.hip gives them."""
    text = open(os.path.join(ROOT, "include", "tnf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(tnf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        names = [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",") if p.strip() != "void"]
        short = {"num_stages": "S", "num_layers": "L", "num_units": "U", "transform_upper": "upper",
                 "params_row_stride": "pstride", "g_params_row_stride": "gpstride"}
        out[name] = [short.get(n, n) for n in names]
        assert len(out[name]) == len(_lib.SIGNATURES[name][1]), name
    return out


BIG = 1 << 40
SCALARS = dict(dtype=0, family=0, M=1, M_z=1, M_p=1, N=4, D=64, S=4, L=2, U=15, H=64, upper=1, inverse=1, ld_mode=0,
               pstride=1000000, gpstride=1000000, workspace_bytes=BIG, fusion=0, rows=4, eps=1e-5, ldh=64, ldw=64,
               ldgh=64, ldgw=64, layer=0, D_in=4, D_attr=5, n=4, ld_eta=1 << 20, key=1, value=0, which=0)
SHAPE = {"tnf_ar_flow_log_prob_bwd_f32": dict(D=6), "tnf_flow_padded_log_prob_f32": dict(D=5),
         "tnf_flow_padded_forward_f32": dict(D=5), "tnf_ef_dot_backward": dict(D=4), "tnf_ef_dot": dict(D=4),
         "tnf_ef_suffstats": dict(D=4), "tnf_ef_suffstats_backward": dict(D=4)}
FLOW_V, LAYER_V, PREC = str(_lib.OPT_FLOW_VARIANT), str(_lib.OPT_LAYER_VARIANT), str(_lib.OPT_OPERAND_PREC)


class Writer(object):
    def __init__(self):
        self.protos = _prototypes()
        self.out = {"query": {}, "query_msg": {}, "reject": {}, "empty": {}}

    def args(self, entry, changes):
        names = self.protos[entry]
        types = _lib.SIGNATURES[entry][1]
        base = {}
        for i, (n, t) in enumerate(zip(names, types)):
            base[n] = 4096 * (i + 1) if t is ctypes.c_void_p else dict(SCALARS, **SHAPE.get(entry, {}))[n]
        base["stream"] = None
        for k, v in changes.items():
            assert k in base, (entry, k)
            if isinstance(v, str):  # "+4": the baseline pointer moved; "=z": the value of another argument
                v = base[k] + int(v) if v[0] == "+" else base[v[1:]]
            base[k] = v
        return [base[n] for n in names]

    def reject(self, entry, code, text, opts=None, kind="reject", **changes):
        args = self.args(entry, changes)
        rc, msg = call(entry, args, opts)
        assert rc == code and (rc >= 0 or text in msg), (entry, changes, opts, rc, msg)
        row = {"args": args, "rc": rc}
        if opts:
            row["opts"] = opts
        if rc < 0:
            row["msg"] = msg
        self.out[kind].setdefault(entry, []).append(row)

    def empty(self, entry, zero, null, null_code=0):
        self.reject(entry, 0, "", kind="empty", **{zero: 0})
        self.reject(entry, null_code, "NULL", kind="empty", **{zero: 0, null: None})


def write():
    w = Writer()
    R, E = w.reject, w.empty
    INV, UNS, WS = -1, -2, -4
    # ---- options and counters ----
    R("tnf_gated_copy_f32", INV, "NULL", flag=None)
    R("tnf_gated_copy_f32", INV, "n=-1", n=-1)
    R("tnf_set_option", INV, "operand precision", key=6, value=2)
    R("tnf_set_option", INV, "reversible-backward", key=7, value=2)
    R("tnf_set_option", INV, "unknown key", key=99, value=1)
    for key in _lib._OPTION_KEYS:
        R("tnf_set_option", 0, "", opts={str(key): _get_option(key)}, key=key, value=_get_option(key))
    R("tnf_get_option", INV, "NULL", value=None)
    R("tnf_get_option", INV, "unknown key", key=99)
    for fam in (-1, _lib.DIAG_FAMILIES):
        w.out["reject"].setdefault("tnf_diag_launch_count", []).append(
            {"args": [fam], "rc": -1, "msg": call("tnf_diag_launch_count", [fam])[1]})
    for which in (-1, 2):
        R("tnf_ef_launch_count", INV, "counter", which=which)

    def mnd(entry):  # check_mnd
        R(entry, INV, "bad batch sizes", M_z=0)
        R(entry, INV, "bad batch sizes", M_p=0)
        R(entry, INV, "bad batch sizes", N=-1)
        R(entry, INV, "do not broadcast", M_z=2, M_p=3)
        R(entry, INV, "must be positive", D=0)

    def triple(entry, text="M="):  # the training batch triple
        R(entry, INV, text, M=0)
        R(entry, INV, text, M=2, M_p=3)
        R(entry, INV, text, N=-1)

    # ---- bijector level ----
    e = "tnf_coupling"
    R(e, INV, "dtype", dtype=7)
    mnd(e)
    R(e, INV, "both halves", D=1)
    R(e, INV, "num_layers", L=0)
    R(e, INV, "num_layers", U=0)
    R(e, INV, "ld_mode", ld_mode=5)
    R(e, INV, "params row has 10", pstride=10)
    for p in ("z", "params", "z_out", "log_det"):
        R(e, INV, "NULL", **{p: None})
    R(e, INV, "alias", z_out="=z")
    R(e, INV, "dtype", kind="reject", dtype=7, D=1, pstride=10, z=None)  # order: the first check wins
    E(e, "N", "z_out", INV)
    e = "tnf_affine"
    R(e, INV, "dtype", dtype=7)
    mnd(e)
    R(e, INV, "params row has 10", pstride=10)
    R(e, INV, "NULL", log_det=None)
    e = "tnf_bn_apply"
    R(e, INV, "dtype", dtype=7)
    R(e, INV, "rows=-1", rows=-1)
    R(e, INV, "D=0", D=0)
    R(e, INV, "NULL", alpha=None)
    e = "tnf_bn_batch_forward_f32"
    R(e, INV, "rows=1", rows=1)
    R(e, INV, "D=0", D=0)
    R(e, INV, "NULL", mean_out=None)
    R(e, INV, "NULL", workspace=None)
    R(e, WS, "workspace 8", workspace_bytes=8)
    for e in ("tnf_coupling_backward", "tnf_coupling_backward_ws", "tnf_maf_backward", "tnf_maf_backward_ws"):
        R(e, INV, "dtype", dtype=7)
        triple(e)
        R(e, INV, "D=%d" % (1 if "coupling" in e else 0), D=1 if "coupling" in e else 0)
        R(e, INV, "L=0", L=0)
        R(e, INV, "U=0", U=0)
        R(e, INV, "shorter than", pstride=10)
        R(e, INV, "shorter than", gpstride=10)
        R(e, INV, "NULL", g_params=None)
        R(e, INV, "NULL", z=None)
        E(e, "N", "g_z", INV)
    R("tnf_coupling_backward_workspace_bytes", INV, "dtype=7", dtype=7)
    R("tnf_coupling_backward_workspace_bytes", INV, "M=2 M_p=3", M=2, M_p=3)
    R("tnf_maf_backward_workspace_bytes", INV, "dtype=7", dtype=7)
    R("tnf_maf_backward_workspace_bytes", INV, "M=0", M=0)
    e = "tnf_affine_backward"
    R(e, INV, "dtype", dtype=7)
    triple(e)
    R(e, INV, "D=0", D=0)
    R(e, INV, "shorter than", pstride=10)
    R(e, INV, "shorter than", gpstride=10)
    R(e, INV, "NULL", params=None)
    R(e, INV, "NULL", z=None)
    e = "tnf_bn_apply_backward"
    R(e, INV, "dtype", dtype=7)
    R(e, INV, "rows=-1", rows=-1)
    R(e, INV, "D=0", D=0)
    R(e, INV, "NULL", alpha=None)
    R(e, INV, "NULL", g_z=None)
    e = "tnf_bn_batch_backward_f32"
    R(e, INV, "rows=1", rows=1)
    R(e, INV, "NULL", z_norm=None)
    R(e, WS, "workspace 8", workspace_bytes=8)
    R("tnf_bn_batch_moments_f32", INV, "rows=-1", rows=-1)
    R("tnf_bn_batch_moments_f32", INV, "NULL", moments=None)
    e = "tnf_bn_batch_normalize_f32"
    R(e, INV, "rows=-1", rows=-1)
    R(e, INV, "NULL", moments=None)
    R(e, INV, "NULL", z=None)
    R(e, WS, "workspace 8", workspace_bytes=8)
    R("tnf_bn_batch_backward_sums_f32", INV, "D=0", D=0)
    R("tnf_bn_batch_backward_sums_f32", INV, "NULL", sums=None)
    R("tnf_bn_batch_backward_apply_f32", INV, "rows=-1", rows=-1)
    R("tnf_bn_batch_backward_apply_f32", INV, "NULL", count=None)
    for e in ("tnf_maf", "tnf_maf_inverse_alpha"):
        R(e, INV, "dtype", dtype=7)
        mnd(e)
        R(e, INV, "L=0" if "alpha" in e else "num_layers=0", L=0)
        R(e, INV, "U=0" if "alpha" in e else "num_units=0", U=0)
        R(e, INV, "params row has 10", pstride=10)
        R(e, INV, "NULL", masks=None)
        E(e, "N", "z_out", INV)
    R("tnf_maf_inverse_alpha", INV, "NULL", alpha_out=None)
    # ---- AR flow ----
    for e in ("tnf_ar_flow_log_prob_f32", "tnf_ar_flow_forward_f32"):
        mnd(e)
        R(e, UNS, "no kernel", D=65)
        R(e, UNS, "no kernel", L=6)
        R(e, INV, "params row has 10", pstride=10)
        R(e, INV, "NULL", bn_mean=None)
        R(e, INV, "NULL", workspace=None)
        R(e, WS, "workspace 8", workspace_bytes=8)
        E(e, "N", "masks", INV)
    R("tnf_ar_flow_log_prob_f32", INV, "no output", log_prob=None, z0=None, sum_log_det=None)
    R("tnf_ar_flow_forward_f32", INV, "NULL", z_out=None)
    R("tnf_ar_flow_forward_f32", INV, "NULL", sum_log_det=None)
    e = "tnf_ar_flow_log_prob_bwd_f32"
    triple(e)
    R(e, UNS, "no kernel", D=40)
    R(e, INV, "shorter than", pstride=10)
    R(e, INV, "shorter than", gpstride=10)
    R(e, INV, "NULL", g_log_prob=None)
    R(e, INV, "NULL", workspace=None)
    R(e, WS, "workspace 8", workspace_bytes=8)
    E(e, "N", "g_params", INV)
    # ---- conditional flow ----
    R("tnf_cond_flow_workspace_bytes", UNS, "no kernel", H=50)
    R("tnf_cond_flow_bwd_workspace_bytes", UNS, "no kernel", H=50)
    for e, first in (("tnf_cond_flow_log_prob_f32", "z"), ("tnf_cond_flow_forward_f32", "omega"),
                     ("tnf_cond_flow_log_prob_fwd_f32", "z"), ("tnf_cond_flow_log_prob_bwd_f32", "acts")):
        R(e, INV, "M=-1", M=-1)
        R(e, UNS, "no kernel", H=50)
        R(e, UNS, "no kernel", U=17)
        R(e, INV, "multiples of 4", ldh=62)
        R(e, INV, "multiples of 4", ldw=32)
        R(e, INV, "NULL", b=None)
        R(e, INV, "aligned", **{first: "+4"})
        R(e, INV, "aligned", h="+8")
        R(e, INV, "aligned", W="+4")
        R(e, INV, "aligned", workspace="+16")
        R(e, WS, "workspace 8", workspace_bytes=8)
        if not e.endswith("bwd_f32"):
            E(e, "M", "b")
    R("tnf_cond_flow_forward_f32", INV, "aligned", z_out="+8")
    R("tnf_cond_flow_log_prob_fwd_f32", INV, "aligned", acts="+4")
    R("tnf_cond_flow_log_prob_fwd_f32", INV, "NULL", acts=None)
    e = "tnf_cond_flow_log_prob_bwd_f32"
    R(e, INV, "ldgh=62", ldgh=62)
    R(e, INV, "ldgw=32", ldgw=32)
    R(e, INV, "NULL", g_W=None)
    R(e, INV, "NULL", g_b=None)
    R(e, INV, "NULL", deltas=None)
    R(e, INV, "aligned", g_h="+4")
    R(e, INV, "aligned", g_z="+8")
    R("tnf_cond_flow_acts_floats", INV, "M=-1", M=-1)
    R("tnf_cond_flow_acts_floats", INV, "D=1", D=1)
    R("tnf_cond_flow_deltas_floats", INV, "H=0", H=0)
    # ---- support layers, exponential families, base density ----
    for e, d in (("tnf_to_interval", "D"), ("tnf_to_interval_backward", "D"), ("tnf_to_simplex", "D_in"),
                 ("tnf_to_simplex_backward", "D_in")):
        R(e, INV, "dtype", dtype=7)
        R(e, INV, "rows=-1", rows=-1)
        R(e, INV, d + "=0", **{d: 0})
        R(e, INV, "NULL", z=None)
        E(e, "rows", "z")
    R("tnf_to_simplex", INV, "D_attr=0", D_attr=0)
    R("tnf_ef_num_eta", INV, "family=5", family=5)
    for e in ("tnf_ef_suffstats", "tnf_ef_suffstats_backward", "tnf_ef_dot", "tnf_ef_dot_backward"):
        R(e, INV, "dtype", dtype=7)
        R(e, INV, "family 5", family=5)
        R(e, INV, "must be positive", D=0)
        R(e, UNS, "exceeds", D=40000)
        R(e, INV, "NULL", z=None)
    R("tnf_ef_suffstats", INV, "rows=-1", rows=-1)
    R("tnf_ef_suffstats_backward", INV, "rows=-1", rows=-1)
    R("tnf_ef_suffstats_backward", INV, "NULL", g_z=None)
    for e in ("tnf_ef_dot", "tnf_ef_dot_backward"):
        R(e, INV, "bad batch sizes", M=-1)
        R(e, INV, "bad batch sizes", N=-1)
        R(e, INV, "ld_eta=1", ld_eta=1)
    R("tnf_ef_dot_backward", WS, "workspace", workspace=None)
    R("tnf_ef_dot_backward", WS, "workspace 0", workspace_bytes=0)
    R("tnf_ef_dot_bwd_workspace_bytes", INV, "M=-1", M=-1)
    R("tnf_ef_dot_bwd_workspace_bytes", INV, "family=5", family=5)
    e = "tnf_base_log_density_f64"
    R(e, INV, "dtype", dtype=7)
    R(e, INV, "rows=-1", rows=-1)
    R(e, INV, "NULL", out=None)
    # ---- coupling flow: inference ----
    R("tnf_flow_workspace_bytes", INV, "M=0", M=0)
    R("tnf_flow_workspace_bytes", INV, "U=0", U=0)
    R("tnf_flow_workspace_bytes", UNS, "no fused kernel", D=6)
    lp = ("tnf_flow_log_prob_f32", "tnf_flow_log_prob_diag_f32")
    fw = ("tnf_flow_forward_f32", "tnf_flow_forward_logq_f32")
    for e in lp + fw:
        mnd(e)
        R(e, INV, "S=0", S=0)
        R(e, INV, "L=0", L=0)
        R(e, INV, "params row has 10", pstride=10)
        R(e, UNS, "no fused kernel", D=6)
        R(e, UNS, "no fused kernel", U=65)
        R(e, UNS, "whole-flow kernel unavailable", fusion=2, S=40)
        R(e, UNS, "whole-flow kernel unavailable", fusion=2, U=20)
        R(e, INV, "fusion 9", fusion=9)
        R(e, WS, "workspace 16", workspace_bytes=16)
        R(e, WS, "workspace", workspace=None)
        R(e, WS, "workspace", fusion=1, workspace_bytes=lib.tnf_flow_workspace_bytes(1, 4, 64, 4, 2, 15, 2))
        R(e, INV, "NULL", bn_alpha=None)
        R(e, INV, "NULL", params=None)
        first = "z" if e in lp else "omega"
        R(e, INV, "aligned", **{first: "+4"})
        R(e, INV, "aligned", **{first: "+8"})
        # a support layer on a route that has none (the refusal precedes every launch)
        R(e, UNS, "support layer", fusion=1, opts={LAYER_V: 0})
        R(e, UNS, "support layer", fusion=2, opts={FLOW_V: 0})
        R(e, UNS, "support layer", fusion=0, U=20)
        R(e, UNS, "support layer", fusion=1, U=20)
        R(e, INV, "must be positive", fusion=9, workspace=None, S=0, D=0)  # order: check_mnd first
    for e in lp:
        R(e, INV, "no output", log_prob=None, z0=None, sum_log_det=None)
        R(e, INV, "aligned", z0="+4")
        R(e, INV, "alias", z0="=z")
        R(e, UNS, "no bf16-operand", U=20, opts={PREC: 1})
        R(e, UNS, "no bf16-operand", U=20, fusion=1, opts={PREC: 1})
        R(e, UNS, "no bf16-operand", U=20, fusion=1, opts={PREC: 1, LAYER_V: 0})  # bf16 is decided before the support layer
        E(e, "N", "z", INV)
    for e in fw:
        R(e, INV, "NULL", z_out=None)
        R(e, INV, "NULL", sum_log_det=None)
        R(e, INV, "aligned", z_out="+4")
        R(e, INV, "alias", z_out="=omega")
        R(e, UNS, "support layer", fusion=1)  # the sampling chain fuses no support layer at any layer variant
        E(e, "N", "omega", INV)
    e = "tnf_flow_forward_logq_f32"
    R(e, INV, "NULL log_q", log_q=None)
    R(e, UNS, "log_q", fusion=1, interval_consts=None)
    R(e, UNS, "log_q", fusion=1, interval_consts=None, opts={LAYER_V: 0})
    R(e, UNS, "log_q", fusion=2, interval_consts=None, opts={FLOW_V: 15})
    R(e, UNS, "log_q", fusion=2, interval_consts=None, opts={FLOW_V: 0})
    R(e, UNS, "log_q", fusion=0, interval_consts=None, S=7)  # whole flow fits, flow_fused2 does not
    R(e, UNS, "log_q", fusion=0, interval_consts=None, U=20)
    R(e, UNS, "log_q", fusion=0, S=7)  # with a support layer the f16 kernel could fuse: still log_q
    R(e, UNS, "support layer", fusion=1)  # order: the support-layer refusal comes before the log_q refusal
    # ---- padded whole-flow kernel ----
    R("tnf_flow_padded_workspace_bytes", INV, "M=0", M=0)
    R("tnf_flow_padded_workspace_bytes", UNS, "no padded kernel", D=64)
    for e, first in (("tnf_flow_padded_log_prob_f32", "z"), ("tnf_flow_padded_forward_f32", "omega")):
        mnd(e)
        R(e, INV, "S=0", S=0)
        R(e, INV, "NULL", **{first: None})
        R(e, INV, "NULL", bn_mean=None)
        R(e, INV, "params row has 10", pstride=10)
        R(e, UNS, "no padded whole-flow kernel", D=64)
        R(e, UNS, "no padded whole-flow kernel", D=32)
        R(e, UNS, "no padded whole-flow kernel", U=17)
        R(e, WS, "workspace 8", workspace_bytes=8)
        R(e, WS, "workspace", workspace=None)
        R(e, INV, "4-byte aligned", **{first: "+2"})
        R(e, INV, "alias", **{"z0" if first == "z" else "z_out": "=" + first})
        E(e, "N", "params", INV)
    R("tnf_flow_padded_log_prob_f32", INV, "no output", log_prob=None, z0=None, sum_log_det=None)
    R("tnf_flow_padded_log_prob_f32", INV, "4-byte aligned", log_prob="+2")
    R("tnf_flow_padded_forward_f32", INV, "NULL", z_out=None)
    R("tnf_flow_padded_forward_f32", INV, "NULL", sum_log_det=None)
    R("tnf_flow_padded_forward_f32", INV, "log_q 8-byte", log_q="+4")
    # ---- coupling flow: training ----
    R("tnf_flow_train_workspace_bytes", INV, "M=0", M=0)
    R("tnf_flow_train_workspace_bytes", INV, "S=0", S=0)
    R("tnf_flow_train_workspace_bytes", UNS, "no training kernels", D=8)
    for e in ("tnf_flow_log_prob_fwd_f32", "tnf_flow_log_prob_bwd_f32"):
        triple(e)
        R(e, INV, "S=0", S=0)
        R(e, UNS, "no training kernels", D=8)
        R(e, UNS, "no training kernels", U=17)
        R(e, INV, "params row has 10", pstride=10)
        R(e, WS, "workspace", workspace=None)
        R(e, WS, "workspace 8", workspace_bytes=8)
        R(e, INV, "NULL", bn_mean=None)
        E(e, "N", "z", INV)
    R("tnf_flow_log_prob_fwd_f32", INV, "aligned", z="+4")
    R("tnf_flow_log_prob_fwd_f32", INV, "aligned", states="+8")
    R("tnf_flow_log_prob_bwd_f32", INV, "g_params row too short", gpstride=10)
    R("tnf_flow_train_rev_workspace_bytes", INV, "M=2 M_p=3", M=2, M_p=3)
    R("tnf_flow_train_rev_workspace_bytes", UNS, "D=8", D=8)
    for e in ("tnf_flow_log_prob_fwd_rev_f32", "tnf_flow_log_prob_bwd_rev_f32"):
        triple(e)
        R(e, UNS, "no reversible training kernels", D=8)
        R(e, UNS, "no reversible training kernels", S=5)
        R(e, INV, "params row has 10", pstride=10)
        R(e, INV, "NULL", bn_alpha=None)
        E(e, "N", "params")
    R("tnf_flow_log_prob_fwd_rev_f32", INV, "aligned", z="+4")
    R("tnf_flow_log_prob_fwd_rev_f32", INV, "aligned", z0="+8")
    e = "tnf_flow_log_prob_bwd_rev_f32"
    R(e, INV, "aligned", z0="+4")
    R(e, INV, "aligned", g_z="+8")
    R(e, INV, "g_params row too short", gpstride=10)
    R(e, WS, "workspace", workspace=None)
    R(e, WS, "workspace 8", workspace_bytes=8)
    # bf16 operands on a shape the reversible pair supports but the all-layers range kernel does not hold in LDS
    R("tnf_flow_log_prob_fwd_rev_f32", UNS, "no bf16-operand", D=32, S=14, L=1, opts={PREC: 1})
    for e in lp:
        R(e, UNS, "no bf16-operand", D=32, S=14, L=1, opts={PREC: 1})
    # ---- batch-statistics chains ----
    R("tnf_flow_forward_batch_workspace_bytes", INV, "M_p=0", M_p=0)
    R("tnf_flow_forward_batch_workspace_bytes", INV, "D=1", D=1)
    e = "tnf_flow_forward_batch_f32"
    triple(e)
    R(e, INV, "S=0", S=0)
    R(e, UNS, "no kernel", D=8)
    R(e, INV, "more than one row", N=1)
    R(e, INV, "params row has 10", pstride=10)
    R(e, INV, "NULL", bn_mean_out=None)
    R(e, INV, "NULL", workspace=None)
    R(e, INV, "aligned", omega="+4")
    R(e, INV, "aligned", z_out="+8")
    R(e, INV, "alias", z_out="=omega")
    R(e, WS, "workspace 8", workspace_bytes=8)
    for e in ("tnf_flow_forward_batch_begin_f32", "tnf_flow_forward_batch_layer_f32", "tnf_flow_forward_batch_fold_f32"):
        R(e, INV, "M_p=0", M_p=0)
        R(e, INV, "S=0", S=0)
        R(e, UNS, "no kernel", D=8)
        R(e, INV, "params row has 10", pstride=10)
        R(e, WS, "workspace", workspace=None)
        R(e, WS, "workspace 8", workspace_bytes=8)
        R(e, INV, "NULL", params=None)
    e = "tnf_flow_forward_batch_layer_f32"
    triple(e)
    R(e, INV, "layer -1 of 8", layer=-1)
    R(e, INV, "layer 8 of 8", layer=8)
    R(e, INV, "NULL", moments=None)
    R(e, INV, "NULL", z_in=None)
    R(e, INV, "aligned", z_in="+4")
    R(e, INV, "aligned", z_out="+8")
    R(e, INV, "aligned", moments="+4")
    R(e, INV, "alias", z_out="=z_in")
    e = "tnf_flow_forward_batch_fold_f32"
    R(e, INV, "layer 8 of 8", layer=8)
    R(e, INV, "NULL", moments=None)
    R(e, INV, "NULL", bn_alpha_out=None)
    e = "tnf_flow_forward_batch_end_f32"
    triple(e)
    R(e, INV, "D=1", D=1)
    R(e, WS, "workspace too small", workspace=None)
    R(e, WS, "workspace too small", workspace_bytes=8)
    R(e, INV, "NULL", z_out=None)
    R("tnf_flow_forward_train_workspace_bytes", INV, "M=2 M_p=3", M=2, M_p=3)
    R("tnf_flow_forward_train_workspace_bytes", INV, "L=0", L=0)
    for e in ("tnf_flow_forward_train_fwd_f32", "tnf_flow_forward_train_bwd_f32"):
        triple(e)
        R(e, INV, "S=0", S=0)
        R(e, UNS, "no kernel", D=8)
        R(e, INV, "more than one row", N=1)
        R(e, INV, "params row has 10", pstride=10)
        R(e, WS, "workspace", workspace=None)
        R(e, WS, "workspace 8", workspace_bytes=8)
        R(e, INV, "NULL", params=None)
        R(e, INV, "aligned", omega="+4")
        R(e, INV, "aligned", states="+8")
    R("tnf_flow_forward_train_fwd_f32", INV, "NULL", folds=None)
    R("tnf_flow_forward_train_fwd_f32", INV, "aligned", z_out="+4")
    e = "tnf_flow_forward_train_bwd_f32"
    R(e, INV, "NULL", g_sum_log_det=None)
    R(e, INV, "g_params row too short", gpstride=10)
    R(e, INV, "aligned", g_omega="+4")
    R(e, INV, "aligned", workspace="+16")
    # ---- small count queries with their rejections ----
    R("tnf_coupling_num_params", INV, "D=0", D=0)
    R("tnf_flow_num_params", INV, "S=0", S=0)
    R("tnf_maf_num_params", INV, "U=0", U=0)
    R("tnf_bn_batch_workspace_bytes", INV, "D=0", D=0)
    R("tnf_ar_flow_workspace_bytes", INV, "M_p=0", M_p=0)
    R("tnf_ar_flow_bwd_workspace_bytes", INV, "D=0", D=0)

    # queries: the answers in grid order; the message of the first failing row of each entry and code (the others
    # differ from it only in the numbers they echo, and every such site has its row among the rejections)
    for i, (entry, args) in enumerate(query_grid()):
        rc, msg = call(entry, args)
        answers = w.out["query"].setdefault(entry, [])
        kept = w.out["query_msg"].setdefault(entry, [])
        if rc < 0 and rc not in [call(entry, GRID[entry][j])[0] for j, _ in kept]:
            kept.append([len(answers), msg])
        answers.append(rc)
    for kind in ("reject", "empty"):
        for rows in w.out[kind].values():
            assert all(r["rc"] != -3 for r in rows), rows
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(
            '"%s": {\n%s\n}' % (kind, ",\n".join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":")))
                                                 for k, v in sorted(w.out[kind].items())))
            for kind in ("query", "query_msg", "reject", "empty")) + "\n}\n")
    table = _table()
    print("query rows:", sum(len(v) for v in table["query"].values()), "reject:", sum(len(v) for v in table["reject"].values()),
          "empty:", sum(len(v) for v in table["empty"].values()), "bytes:", os.path.getsize(TABLE))


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_cabi_host_table.py --write")
    write()
