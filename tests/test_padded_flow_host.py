"""Host-side checks of the whole-flow kernel's padded layouts (tnf_flow_padded_*): the support predicate and its LDS
limits, the workspace size, and every argument check -- each refusal returns its code and message without launching
(no device is touched: the checks run before any HIP call)."""
import ctypes

import pytest
import torch

from torch_nf_amd import _lib as L_

lib = L_.lib
EINVAL, EWORKSPACE = -1, -4  # include/tnf.h

# S_max per (H, L): the flow2_lds_bytes accounting of the D = 2H kernel plus the staging tiles of the padded layout
# (12 waves x 16 rows x 32 floats at H = 16, 8 waves x 16 rows x 64 floats at H = 32), within 160 KB of LDS
S_MAX = {(16, 1): 14, (16, 2): 9, (16, 3): 7, (32, 1): 6, (32, 2): 5, (32, 3): 4}
DS = (2, 3, 4, 5, 7, 8, 15, 16, 17, 24, 31, 33, 40, 47, 48, 63)


def half(D):
    return 16 if D <= 31 else 32


def s_max(D, L, U):
    S = 0
    while lib.tnf_flow_padded_supported(D, S + 1, L, U):
        S += 1
        assert S < 100
    return S


@pytest.mark.parametrize("U", [15, 16])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_supported_s_max_pinned_and_monotone(L, U):
    for D in DS:
        S = s_max(D, L, U)
        assert S == S_MAX[half(D), L], (D, L, U, S)
        for s in range(1, S + 1):
            assert lib.tnf_flow_padded_supported(D, s, L, U) == 1
        for s in range(S + 1, S + 6):
            assert lib.tnf_flow_padded_supported(D, s, L, U) == 0
        assert lib.tnf_flow_padded_supported(D, 0, L, U) == 0


def test_supported_refusals():
    for D in (0, 1, 32, 64, 65, 100):
        for L in (1, 2, 3):
            assert lib.tnf_flow_padded_supported(D, 1, L, 15) == 0, D
    for D in (2, 5, 47, 63):
        assert lib.tnf_flow_padded_supported(D, 1, 4, 15) == 0
        assert lib.tnf_flow_padded_supported(D, 1, 0, 15) == 0
        assert lib.tnf_flow_padded_supported(D, 1, 2, 17) == 0
        assert lib.tnf_flow_padded_supported(D, 1, 2, 0) == 0
        assert lib.tnf_flow_padded_supported(D, 1, 2, 1) == 1
    # the existing predicates keep their answers for these shapes
    assert lib.tnf_has_fast_path(5, 2, 15) == 0
    assert lib.tnf_flow_fused_supported(5, 4, 2, 15) == 0 and lib.tnf_flow_fused2_supported(8, 4, 2, 15) == 0


def test_workspace_bytes():
    prev = 0
    for M in (1, 2, 3, 100, 10 ** 5):
        b = lib.tnf_flow_padded_workspace_bytes(M, 1000, 5, 4, 2, 15)
        assert b > prev and b % 16 == 0
        prev = b
    assert lib.tnf_flow_padded_workspace_bytes(1, 0, 5, 4, 2, 15) > 0
    assert lib.tnf_flow_padded_workspace_bytes(0, 10, 5, 4, 2, 15) == EINVAL
    assert lib.tnf_flow_padded_workspace_bytes(1, 10, 32, 4, 2, 15) == L_.EUNSUPPORTED
    assert lib.tnf_flow_padded_workspace_bytes(1, 10, 5, 4, 2, 17) == L_.EUNSUPPORTED


def _err():
    return lib.tnf_last_error().decode()


class _Args:
    """Fake (never dereferenced) pointers: every call below must be refused before it launches anything."""

    def __init__(self, D=5, S=2, L=2, U=15, Mz=1, Mp=1, N=100):
        self.D, self.S, self.L, self.U, self.Mz, self.Mp, self.N = D, S, L, U, Mz, Mp, N
        self.P = lib.tnf_flow_num_params(D, S, L, U)
        self.ws_bytes = lib.tnf_flow_padded_workspace_bytes(max(Mz, Mp), N, D, S, L, U)
        self.z, self.p, self.mean, self.alpha = 0x10000, 0x20000, 0x30000, 0x40000
        self.lp, self.z0, self.sld, self.ws = 0x50000, 0x60000, 0x70000, 0x80000
        self.lq = 0x90000

    def log_prob(self, **kw):
        a = dict(z=self.z, p=self.p, mean=self.mean, alpha=self.alpha, lp=self.lp, z0=self.z0, sld=self.sld,
                 Mz=self.Mz, Mp=self.Mp, N=self.N, D=self.D, S=self.S, L=self.L, U=self.U, pstride=self.P,
                 ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return lib.tnf_flow_padded_log_prob_f32(a["z"], a["p"], a["mean"], a["alpha"], a["lp"], a["z0"], a["sld"],
                                                a["Mz"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"],
                                                a["pstride"], a["ws"], a["ws_bytes"], None, None)

    def forward(self, **kw):
        a = dict(z=self.z, p=self.p, mean=self.mean, alpha=self.alpha, zo=self.z0, sld=self.sld, lq=self.lq,
                 Mz=self.Mz, Mp=self.Mp, N=self.N, D=self.D, S=self.S, L=self.L, U=self.U, pstride=self.P,
                 ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return lib.tnf_flow_padded_forward_f32(a["z"], a["p"], a["mean"], a["alpha"], a["zo"], a["sld"], a["lq"],
                                               a["Mz"], a["Mp"], a["N"], a["D"], a["S"], a["L"], a["U"],
                                               a["pstride"], a["ws"], a["ws_bytes"], None)


def _launches():
    return [lib.tnf_diag_launch_count(f) for f in range(L_.DIAG_FAMILIES)]


@pytest.mark.parametrize("entry", ["log_prob", "forward"])
def test_argument_checks_return_codes_without_launching(entry):
    a = _Args()
    call = getattr(a, entry)
    fn = "tnf_flow_padded_" + ("log_prob_f32" if entry == "log_prob" else "forward_f32")
    out_key = "z0" if entry == "log_prob" else "zo"
    before = _launches()
    cases = [
        (dict(z=None), EINVAL, "NULL pointer"),
        (dict(p=None), EINVAL, "NULL pointer"),
        (dict(mean=None), EINVAL, "NULL pointer"),
        (dict(alpha=None), EINVAL, "NULL pointer"),
        (dict(pstride=a.P - 1), EINVAL, "params row has"),
        (dict(D=32, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(D=64, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(D=1, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(U=17, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(L=4, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(S=S_MAX[16, 2] + 1, pstride=10 ** 6), L_.EUNSUPPORTED, "no padded whole-flow kernel"),
        (dict(ws_bytes=a.ws_bytes - 1), EWORKSPACE, "workspace"),
        (dict(ws=None), EWORKSPACE, "workspace"),
        (dict(Mz=2, Mp=3), EINVAL, "do not broadcast"),
        (dict(N=-1), EINVAL, "bad batch sizes"),
        (dict(z=a.z + 2), EINVAL, "4-byte aligned"),
        ({out_key: a.z}, EINVAL, "must not alias"),
    ]
    if entry == "log_prob":
        cases.append((dict(lp=None, z0=None, sld=None), EINVAL, "no output requested"))
        cases.append((dict(lp=a.lp + 1), EINVAL, "4-byte aligned"))
    else:
        cases.append((dict(zo=None), EINVAL, "NULL pointer"))
        cases.append((dict(sld=None), EINVAL, "NULL pointer"))
        cases.append((dict(lq=a.lq + 4), EINVAL, "aligned"))
    for kw, code, msg in cases:
        rc = call(**kw)
        assert rc == code, (kw, rc, _err())
        assert fn in _err() and msg in _err(), (kw, _err())
    # N == 0 is a no-op that succeeds (with every argument otherwise valid)
    assert call(N=0, ws_bytes=lib.tnf_flow_padded_workspace_bytes(1, 0, a.D, a.S, a.L, a.U)) == 0
    # a 4-byte aligned z (odd float offset) passes the alignment check: refused later only for the workspace
    assert call(z=a.z + 4, ws_bytes=a.ws_bytes - 1) == EWORKSPACE
    assert _launches() == before, "a refused call launched kernels"


def test_declared_in_header_and_bound():
    raw = ctypes.CDLL(L_.LIB_PATH)
    for n in ("tnf_flow_padded_supported", "tnf_flow_padded_workspace_bytes", "tnf_flow_padded_log_prob_f32",
              "tnf_flow_padded_forward_f32"):
        assert hasattr(raw, n) and n in L_.SIGNATURES
    assert (L_.DIAG_FLOW_PADDED, L_.DIAG_FLOW_PADDED_FWD, L_.DIAG_FAMILIES) == (16, 17, 19)


def test_routing_predicate_host_side():
    """NormFlow._padded_ok: the conditions of the issue, checked on CPU tensors (no launch)."""
    import torch_nf_amd as tnf

    nf = tnf.NormFlow(5, False, "coupling", 2, 2, 15)
    z = torch.zeros(1, 40, 5)
    p = nf.params.detach()
    assert nf._padded_ok(z, p)
    assert not nf._padded_ok(z.double(), p)
    assert not nf._padded_ok(z[0], p)
    pp = p.expand(3, -1)
    assert nf._padded_ok(torch.zeros(3, 32, 5), pp) and not nf._padded_ok(torch.zeros(3, 31, 5), pp)
    nf.fusion = L_.FUSE_LAYER
    assert not nf._padded_ok(z, p)
    nf.fusion = L_.FUSE_FLOW
    assert nf._padded_ok(z, p)
    with torch.enable_grad():
        assert not nf._padded_ok(z, p.clone().requires_grad_(True))
    assert not tnf.NormFlow(5, False, "coupling", 2, 2, 20)._padded_ok(z, tnf.NormFlow(5, False, "coupling", 2, 2, 20).params)
    assert not tnf.NormFlow(32, False, "coupling", 2, 2, 15)._padded_ok(torch.zeros(1, 40, 32),
                                                                       tnf.NormFlow(32, False, "coupling", 2, 2, 15).params)
    assert not tnf.NormFlow(5, False, "AR", 2, 2, 15)._padded_ok(z, tnf.NormFlow(5, False, "AR", 2, 2, 15).params)
