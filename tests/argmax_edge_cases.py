"""The table of inputs on which an arg-max can break its rule without its values being wrong: exact ties, signed zeros, denormals,
infinities and NaN.  Shared by tests/test_first_max_cpu.py (the rule of tests/first_max.py against the oracle's restatements, and the
negative controls: a wrong rule must move picks on this table) and tests/test_first_maximum_gpu.py (the env kernel's greedy pick on
finished rows and on the slab forms of the head, and the Double-DQN action of every arg-max implementation of a TD step).  Test
infrastructure only, in the style of tests/td_edge_cases.py: nothing here is imported from the library or the oracle.

The layout rules of the Double-DQN part restate the library's accumulator layout as plain arithmetic (which rows of the 8100 one lane,
one half-wave, one 32-row tile, one wave row, one block tile and one range of partial rows hold); a layout that moves only makes a pair
test another boundary than its comment says, it cannot make a test pass wrongly.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
DENORM = float(np.float32(2.0) ** -149)                 # the smallest positive fp32 denormal


# ---- Q-row patterns for the pick ---------------------------------------------------------------------------------------------------------
# A pattern is a function of a game's legal list (codes, in list order; destination = code % 90) so that the interesting value lands
# on listed squares; it returns the 90 floats of the row, or None where the list has no such entries (tie_two across the halves of
# the 128-entry list needs more than 64 moves).
def _firsts(dests):
    """list indices whose destination no earlier entry reaches: the entries a tie can be decided between"""
    seen, out = set(), []
    for k, d in enumerate(dests):
        if int(d) not in seen:
            seen.add(int(d))
            out.append(k)
    return out


def _base(rng):
    """90 distinct finite values below every value a pattern plants"""
    return rng.permutation(90).astype(F32) * F32(0.01) - F32(0.95)       # -0.95 .. -0.06


def _two(dests, rng, lo_i, hi_i, lo_j, hi_j):
    f = _firsts(dests)
    last_j = max([k for k in f if lo_j <= k < hi_j], default=-1)
    ii = [k for k in f if lo_i <= k < hi_i and k < last_j]
    if not ii:
        return None
    i = ii[int(rng.integers(len(ii)))]
    jj = [k for k in f if lo_j <= k < hi_j and k > i]
    if not jj:
        return None
    return i, jj[int(rng.integers(len(jj)))]


def _tie_all(dests, rng):
    return np.full(90, 0.25, F32)


def _tie_two(lo_i, hi_i, lo_j, hi_j):
    def f(dests, rng):
        ij = _two(dests, rng, lo_i, hi_i, lo_j, hi_j)
        if ij is None:
            return None
        q = _base(rng)
        q[dests[ij[0]]] = q[dests[ij[1]]] = F32(0.5)
        return q
    return f


def _tie_shared_dest(dests, rng):
    d, cnt = np.unique(dests, return_counts=True)
    if not (cnt > 1).any():
        return None
    q = _base(rng)
    q[d[cnt > 1][int(rng.integers((cnt > 1).sum()))]] = F32(0.5)
    return q


def _zeros_signed(first):
    def f(dests, rng):
        ij = _two(dests, rng, 0, 128, 0, 128)
        if ij is None:
            return None
        q = _base(rng)
        q[dests[ij[0]]], q[dests[ij[1]]] = F32(first), F32(-first)       # -0.0 == +0.0: the earlier entry wins either way
        return q
    return f


def _denormals(sign):
    def f(dests, rng):
        q = (rng.permutation(90) + 1).astype(np.float64) * DENORM * sign
        fs = _firsts(dests)
        if len(fs) < 2:
            return None
        best = max(fs, key=lambda k: q[dests[k]])
        if best == 0:                                                    # the largest must not be the first entry
            other = dests[fs[1 + int(rng.integers(len(fs) - 1))]]
            q[dests[0]], q[other] = q[other], q[dests[0]]
        q = q.astype(F32)
        assert len(np.unique(q)) == 90 and (q != 0).all() and (np.abs(q) < np.finfo(F32).tiny).all()
        return q
    return f


def _inf_pos(dests, rng):
    ij = _two(dests, rng, 0, 128, 0, 128)
    if ij is None:
        return None
    q = _base(rng)
    q[dests[ij[0]]] = q[dests[ij[1]]] = F32(np.inf)
    return q


def _inf_neg_rest(dests, rng):
    fs = _firsts(dests)
    if len(fs) < 2:
        return None
    q = np.full(90, -np.inf, F32)
    q[dests[fs[1 + int(rng.integers(len(fs) - 1))]]] = F32(-0.75)
    return q


def _nan_on_best(dests, rng):
    fs = _firsts(dests)
    if len(fs) < 2:
        return None
    q = _base(rng)
    q[dests[fs[int(rng.integers(len(fs)))]]] = F32(0.5)                  # the square that would win ...
    q[q == F32(0.5)] = F32(np.nan)                                       # ... holds a NaN: the finite runner-up wins
    return q


def _nan_all(dests, rng):
    return np.full(90, np.nan, F32)


def _neginf_all(dests, rng):
    return np.full(90, -np.inf, F32)


def _nan_and_neginf(dests, rng):
    q = np.full(90, np.nan, F32)
    q[dests[0]] = -np.inf                                                # entry 0 is no NaN: "NaN wins" moves the pick
    q[rng.permutation(90)[:30]] = -np.inf
    if np.isinf(q[dests]).all():
        q[dests[-1]] = np.nan
    return q


def _sat_one(dests, rng):
    fs = _firsts(dests)
    if len(fs) < 3:
        return None
    q = _base(rng)
    for k in rng.permutation(fs)[:3]:
        q[dests[k]] = F32(1.0)
    return q


Q_PATTERNS = {
    "tie_all": _tie_all,
    "tie_two_first_half": _tie_two(0, 64, 0, 64),
    "tie_two_across_halves": _tie_two(0, 64, 64, 128),
    "tie_two_second_half": _tie_two(64, 128, 64, 128),
    "tie_shared_dest": _tie_shared_dest,
    "zeros_signed_minus_first": _zeros_signed(-0.0),
    "zeros_signed_plus_first": _zeros_signed(0.0),
    "denormals": _denormals(1.0),
    "denormals_negated": _denormals(-1.0),
    "inf_pos": _inf_pos,
    "inf_neg_rest": _inf_neg_rest,
    "nan_on_best": _nan_on_best,
    "nan_all": _nan_all,
    "neginf_all": _neginf_all,
    "nan_and_neginf": _nan_and_neginf,
    "sat_one": _sat_one,
}
LONG_LIST_ONLY = ("tie_two_across_halves", "tie_two_second_half")        # need an entry at or above 64


def q_row(name, codes, seed):
    """the row of pattern `name` for one game (codes: its legal list); None where the pattern does not apply; an empty list: tie_all"""
    dests = np.asarray(codes, dtype=np.int64) % 90
    if len(dests) == 0:
        return np.full(90, 0.25, F32)
    return Q_PATTERNS[name](dests, np.random.default_rng([seed, list(Q_PATTERNS).index(name)]))


def q_rows(name, lists, seed=0):
    """(rows [n][90] float32, applies [n]) of pattern `name` over the games' legal lists; a game the pattern does not apply to gets
    the tie_all row, so that every game of a batch is still checked"""
    q = np.full((len(lists), 90), 0.25, F32)
    ok = np.zeros(len(lists), bool)
    for g, codes in enumerate(lists):
        r = q_row(name, codes, seed * 100003 + g)
        if r is not None:
            q[g], ok[g] = r, len(codes) > 0
    return q, ok


# ---- head patterns for the slab forms ----------------------------------------------------------------------------------------------------
# Edits of output rows 0..89 of a net, in place on W [>= 90][Hl] and b [>= 90] (float64 parameters as DQN.set_params takes them).
def _head_dup_sets(W, b, rng):
    p = rng.permutation(90).reshape(30, 3)                               # 30 sets of three rows: weights and bias both copied
    for s in p:
        W[s[1:]], b[s[1:]] = W[s[0]], b[s[0]]


def _head_all_equal(W, b, rng):
    W[1:90], b[1:90] = W[0], b[0]


def _head_zero_signed(W, b, rng):
    W[:90] = 0.0
    b[:90] = np.where(np.arange(90) % 2 == 0, -0.0, 0.0)


def _head_sat50(W, b, rng):
    W[:90] *= 50.0
    b[:90] *= 50.0


def _head_inf_weight(W, b, rng):
    W[40, int(rng.integers(W.shape[1]))] = np.inf


def _head_nan_weight(W, b, rng):
    W[40, int(rng.integers(W.shape[1]))] = np.nan


HEAD_PATTERNS = {"dup_sets": _head_dup_sets, "all_equal": _head_all_equal, "zero_signed": _head_zero_signed, "sat50": _head_sat50,
                 "inf_weight": _head_inf_weight, "nan_weight": _head_nan_weight}
SLAB_NETS = {"128-128-8100": "rides, 2 slabs", "128-512-8100": "8 slabs, prefetched", "128-640-8100": "10 slabs, loaded late",
             "128-8100": "nothing rides, finished rows"}
L0_SCALE = 10.0          # layer 0 of the slab nets' U(-0.05, 0.05) weights scaled so that hidden activations are O(1) and a x50 head saturates


def edit_head(name, sizes, w, b, seed=0):
    """copies of the flat parameters (w, b) with head pattern `name` applied to output rows 0..89"""
    w, b = np.array(w, dtype=np.float64), np.array(b, dtype=np.float64)
    Hl, NO = sizes[-2], sizes[-1]
    W = w[len(w) - NO * Hl:].reshape(NO, Hl)
    B = b[len(b) - NO:]
    HEAD_PATTERNS[name](W, B, np.random.default_rng([seed, list(HEAD_PATTERNS).index(name)]))
    return w, b


# ---- row positions for Double DQN -----------------------------------------------------------------------------------------------------------
# The arg-max over the 8100 outputs is assembled per lane (16 rows of a 32-row tile: four runs of 4 consecutive rows, 8 apart; the two
# half-waves hold the runs 4 apart), across the half-waves, across the 32-row tiles and the wave rows of a block tile (64 rows per wave
# row, 128 per block tile), and across the partial rows in colmax_reduce_kernel (kReduceParts ranges) and the TD-delta kernel.  A set
# of positions holds copies of ONE output row (weights and bias): the lowest must win.
ROW_SETS = [
    ("same_lane_next", (1201, 1202)),                   # j, j + 1: consecutive registers of one lane
    ("same_lane_8", (2310, 2318)),                      # j, j + 8: the next run of the same lane
    ("half_waves", (3002, 3006)),                       # j, j + 4: the other half-wave
    ("tiles_32", (4005, 4037)),                         # j, j + 32: the next 32-row tile of the wave
    ("wave_rows", (5003, 5067)),                        # j, j + 64: the other wave row / chunk
    ("block_tiles", (6001, 6129)),                      # j, j + 128: the next block tile
    ("row_ranges_a", (5, 4101)),                        # across the ranges of partial rows and the walk's blocks
    ("row_ranges_b", (3, 8099)),
    ("last_group_a", (8096, 8099)),                     # the padded last group (8100 = 63 * 128 + 36)
    ("last_group_b", (8070, 8099)),
    ("triple", (17, 49, 4113)),
]
N_BASE = 8
SHIFT = 4.0                                             # taken off the bias of every other row: it never wins
GAMMA = 0.99


def layouts():
    """Every layout gives each of the eight base rows one set of positions; the three together give every set a base row of its own
    (two sets on one base row would leave the higher one untested; row 8099 is in three sets, so they need three layouts).  The third
    also holds the zero rows, on base row 0."""
    sets = [s[1] for s in ROW_SETS]
    more = [(1203, 1204), (2311, 2319), (3003, 3007), (4006, 4038), (5004, 5068), (6003, 6131)]      # the same boundaries once more
    out = {"sets_0_7": sets[:8], "sets_8_10": [sets[8], sets[10]] + more, "zero_rows": [sets[0], sets[9]] + more}
    for name, lay in out.items():
        flat = [p for s in lay for p in s]
        assert len(lay) == N_BASE and len(set(flat)) == len(flat), name
    return out


ZERO_SET, ZERO_SIGNS = (2050, 2054, 6002), (-0.0, 0.0, -0.0)     # base row 0 of "zero_rows": weights 0, biases -0, +0, -0
ZERO_OTHERS = -3.0                                               # added to the other base rows' biases there: zero wins often


def base_rows(Hl, seed, scale=1.0):
    rng = np.random.default_rng([seed, Hl, 77])
    return rng.uniform(-1.0, 1.0, size=(N_BASE, Hl)) * scale, rng.uniform(-0.5, 0.5, size=N_BASE)


def online_head(layout_name, NO, Hl, seed, nonfinite=None, base_bias=None):
    """(W [NO][Hl], b [NO], the base rows, positions per base row, expected-row override) of the online head for a layout.
    nonfinite: None | "inf_two" | "neginf_first" | "nan_first" | "nan_row0" (biases only; see the GPU test).  base_bias: biases of
    the eight base rows in place of the random ones (the tests centre every base value over the batch: each row then wins often)."""
    lay = [tuple(s) for s in layouts()[layout_name]]
    Wb, bb = base_rows(Hl, seed)
    if base_bias is not None:
        bb = np.array(base_bias, dtype=np.float64)
    if layout_name == "zero_rows":
        Wb[0], bb[0] = 0.0, 0.0
        bb[1:] += ZERO_OTHERS
        lay[0] = ZERO_SET
    rows = np.arange(NO) % N_BASE
    W, b = Wb[rows].copy(), bb[rows] - SHIFT
    for r, pos in enumerate(lay):
        for p in pos:
            W[p], b[p] = Wb[r], bb[r]
    if layout_name == "zero_rows":
        for p, s in zip(ZERO_SET, ZERO_SIGNS):
            b[p] = s
    force = None
    if nonfinite == "inf_two":
        b[[2500, 7000]] = np.inf
        force = 2500                                                 # +inf on two rows: the lower row wins in every sample
    elif nonfinite in ("neginf_first", "nan_first"):
        for r, pos in enumerate(lay):
            assert pos[0] >= 1
            b[pos[0]] = -np.inf if nonfinite == "neginf_first" else np.nan
            lay[r] = pos[1:]                                         # the row that would win never does: the next copy wins
    elif nonfinite == "nan_row0":
        b[0] = np.nan                                                # a NaN in output 0 never wins either
    return W, b, (Wb, bb), lay, force


def target_bias(NO):
    """bias of the target head (its weights are exactly 0): y = gamma tanh(bias[a*]) names a* to within a tanhf rounding"""
    return np.arctanh(-0.97 + 1.94 * np.arange(NO) / (NO - 1))


def decode_astar(y, NO):
    """(nearest row, residual |y - gamma tanh(fp32 bias[row])|) for the device's y of a sample with r = 0"""
    grid = GAMMA * np.tanh(target_bias(NO).astype(np.float32).astype(np.float64))
    y = np.asarray(y, dtype=np.float64)
    k = np.clip(np.searchsorted(grid, y), 1, NO - 1)
    k = np.where(np.abs(grid[k - 1] - y) <= np.abs(grid[k] - y), k - 1, k)
    return k, np.abs(grid[k] - y)


DdqnCase = namedtuple("DdqnCase", "name sizes prec n path tails seed")
_A, _B = [1260, 256, 256, 8100], [1260, 512, 512, 8100]
# path: tile = launch_gemm's tile kernel epilogue (epilogue_colmax with partial_idx); walk = the persistent CM_ARG kernel;
# screen = screen_top2_kernel in SCR_ARG (scr_fold); the TD-delta kernel's generic reduction, or its H == 512 branch for _B.
# tails: the fused tail on / off where it changes the launch the TD-delta text runs in (fp32 nets; a bf16 net never takes the tail)
DDQN_CASES = [
    DdqnCase("f32_n300_tile", _A, 0, 300, "tile", (True, False), 0),
    DdqnCase("f32_n1024_walk", _A, 0, 1024, "walk", (True, False), 1),
    DdqnCase("bf16_n256_pairs", _A, 1, 256, "tile", (True,), 2),
    DdqnCase("bf16_n300_tile_pairs", _A, 1, 300, "tile", (True,), 3),
    DdqnCase("bf16_n1024_screen_frag", _A, 1, 1024, "screen", (True,), 4),
    DdqnCase("bf16_n1100_screen", _A, 1, 1100, "screen", (True,), 5),
    DdqnCase("bf16_h512_n1024", _B, 1, 1024, "screen", (True,), 6),
]
NONFINITE = ("inf_two", "neginf_first", "nan_first", "nan_row0")


def rowmax_path(c):
    """which product leaves the partial maxima of a Double-DQN step (qmax_exact), restated: screen for a bf16 net with a 256- or
    512-wide last hidden layer from 1024 samples on; else the persistent walk when 64 x ceil(n / 128) >= 512 tiles; else the tile kernel"""
    Hl, NO = c.sizes[-2], c.sizes[-1]
    if c.prec != 0 and Hl in (256, 512) and c.n >= 1024:
        return "screen"
    return "walk" if ((NO + 127) // 128) * ((c.n + 127) // 128) >= 512 else "tile"


def walk_bytes(c):
    """the bytes the persistent walk's gemm_qmax_rowmax bracket is recorded with"""
    Hl, NO = c.sizes[-2], c.sizes[-1]
    return (2.0 if c.prec else 4.0) * (NO * Hl + c.n * Hl) + 8.0 * ((NO + 127) // 128) * c.n
