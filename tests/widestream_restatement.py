"""What the streamed whole-flow wide tests share (tests/test_wide_stream_host.py, tests/test_gpu_wide_stream.py): the
predicate, LDS sizes and tile rule of csrc/wide_stream.h restated, and the sweep's shapes.  The kernel's arithmetic is
that of csrc/flow_wide.hip, whose restatement (tests/wideflow_restatement.py: wide_flow_log_prob, wide_flow_forward, Case)
holds at any S.  A helper: no test in here."""
import wideflow_restatement as W

MAX_S = 1024  # kWideStreamMaxS
WAVES, CUS = 8, 256  # WS_WAVES; the budget of persistent_bx(groups, 1, 256, M)
SHIPPED_TILES = (1, 2, 4)


def in_domain(D, L, U):
    return 2 <= D <= 64 and 1 <= L <= 5 and 17 <= U <= 64 and 4 * W.layer_floats(D, L, U) <= W.LDS_BUDGET


def supported(D, S, L, U):
    return 1 <= S <= MAX_S and in_domain(D, L, U)


def slots(D, L, U):
    if not in_domain(D, L, U):
        return 0
    return 2 if 8 * W.layer_floats(D, L, U) <= W.LDS_BUDGET else 1


def lds_bytes(D, L, U):
    return 4 * slots(D, L, U) * W.layer_floats(D, L, U) if in_domain(D, L, U) else 0


def groups(N, T):
    return ((N + 15) // 16 + WAVES * T - 1) // (WAVES * T)


def max_tiles(D, L, U):
    """wide_stream_max_tiles: the largest T instantiated for the tile shape."""
    return (1 if L > 3 else 2) if W.tiles(D, U) == (2, 4) else 4


def tiles(D, L, U, M, N):
    """wide_stream_tiles: the largest T of the shape with M groups(N, T) >= 256 and ceil(N / 16) > 8 (T / 2), else 1."""
    T = max_tiles(D, L, U)
    while T > 1:
        if groups(N, T) >= (CUS + M - 1) // M and (N + 15) // 16 > WAVES * (T // 2):
            return T
        T //= 2
    return 1


def grid_x(N, M, T):
    return min(groups(N, T), max(1, CUS // M))


# ---- the sweep: none of these is accepted by tnf_wide_flow_supported ---------------------------------------------------------
SWEEP = [(3, 9, 1, 32), (33, 9, 1, 17), (63, 5, 1, 32),
         (2, 5, 2, 20), (4, 5, 2, 20), (5, 9, 2, 17), (31, 3, 2, 48), (33, 3, 2, 20), (64, 4, 2, 64),
         (64, 1, 3, 64), (32, 2, 3, 64),
         (5, 3, 4, 20), (64, 2, 4, 33),
         (31, 2, 5, 20), (8, 2, 5, 64), (64, 1, 5, 48)]
ONE_SLOT = [(64, 1, 3, 64), (32, 2, 3, 64), (64, 2, 4, 33), (8, 2, 5, 64), (64, 1, 5, 48)]
BOTH = [(5, 1, 2, 20), (33, 2, 2, 20), (64, 1, 2, 64), (8, 1, 5, 20)]  # accepted by the resident kernel too
WALK_SHAPES = [(5, 5, 2, 20), (33, 3, 2, 20)]
WALK_M = 129


def walk_N(T):
    """Three groups of 8 T tiles, the last holding one full tile and one row."""
    return 2 * 128 * T + 17


NF_SHAPE = (64, 4, 2, 64)   # NormFlow(64, False, 'coupling', 4, 2, 64): the headline model with 64 units
CDE_SHAPE = (4, 5, 2, 20)   # NormFlow(4, True, 'coupling', 5, 2, 20) inside a ConditionalDensityEstimator
