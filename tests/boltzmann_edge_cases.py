"""The inputs of the Boltzmann-pick tests, shared by tests/test_boltzmann_ref_cpu.py (the reference against the analytic softmax, an fp32
emulation of the device rule and the negative controls) and tests/test_boltzmann_gpu.py (the env kernel on the same boards, rows and
Philox words).  Test infrastructure only: the legal lists come from the oracle, nothing from the library.

2048 games from tests/sparse_boards.gen_arbitrary: two boards of every legal-list length in SPECIAL_LENGTHS (0, 1, 2, the lengths
around the 64-lane boundary and the longest list the generator gives, which needs the second scan) once under every row pattern, then
the generator's boards in order.  Game g gets row pattern g mod len(ROW_PATTERNS): the patterns of tests/argmax_edge_cases.py (exact
ties, signed zeros, denormals, +-inf, NaN) and four of this file's own (rows outside [-1, 1] among them).  The Philox words are the env
kernel's: ctr = {ply counter of the slot (0 after set_state), 0, first_game_id + g, 0}, key = seed.
"""
import numpy as np

import argmax_edge_cases as ac
import boltzmann_ref as bz
import sparse_boards as sb
import xqoracle as xo

F32 = np.float32
N_GAMES = 2048
SEED = 0x5EED + 73
TEMPS = (0.05, 0.25, 1.0, 4.0)
SPECIAL_LENGTHS = (0, 1, 2, 63, 64, 65)
EPS_COMPOSED = 0.3
# words that put t on a prefix sum exactly (u = 0, 1/4, 1/2, 3/4) or next to the total: only the CPU tests can choose a word
CRAFTED_R2 = (0, 1 << 30, 1 << 31, 3 << 30, 0xFFFFFFFF, 0xFFFFFF00, 0x000000FF)


def _uniform(dests, rng):
    return rng.uniform(-1.0, 1.0, 90).astype(F32)


def _wide(dests, rng):
    """outside [-1, 1]: at T = 0.05 the largest x_i pass -104 (exact zero weights) and exp(v / T) without the maximum taken off
    overflows"""
    return rng.uniform(-6.0, 6.0, 90).astype(F32)


def _clusters(dests, rng):
    """two groups of exactly equal values 0.1 apart: many equal weights, boundaries evenly spaced"""
    return np.where(rng.random(90) < 0.5, F32(0.3), F32(0.2)).astype(F32)


def _one_ahead(dests, rng):
    """a unique maximum far ahead of the rest: at a small T every draw is the first maximum"""
    q = (rng.uniform(-1.0, -0.5, 90)).astype(F32)
    q[dests[int(rng.integers(len(dests)))]] = F32(0.9)
    return q


ROW_PATTERNS = dict(ac.Q_PATTERNS)
ROW_PATTERNS.update(uniform=_uniform, wide=_wide, clusters=_clusters, one_ahead=_one_ahead)
PATTERN_NAMES = list(ROW_PATTERNS)

_cache = {}


def inputs():
    """-> dict(boards [n][90] u8, meta [n][4] i32, lists [n] of codes, q [n][90] f32, pattern [n] names, longest)"""
    if "in" in _cache:
        return _cache["in"]
    B, M = sb.gen_arbitrary(4000, 7)
    L = []
    for s, m in zip(B, M):
        codes, cnt = xo.all_valid_actions(xo.board_from(s, *m), int(m[1]))
        assert cnt <= 128
        L.append(codes[:cnt])
    n_of = np.array([len(c) for c in L])
    longest = int(n_of.max())
    assert longest > 64
    order = []
    for length in SPECIAL_LENGTHS + (longest,):
        have = np.nonzero(n_of == length)[0][:2]
        assert len(have) >= 1, length
        for b in have:
            order += [int(b)] * len(PATTERN_NAMES)               # consecutive games: one of every pattern
    order += list(range(N_GAMES - len(order)))
    order = np.array(order[:N_GAMES])
    boards, meta, lists = B[order], M[order], [L[i] for i in order]
    q = np.zeros((N_GAMES, 90), F32)
    pattern = []
    for g, codes in enumerate(lists):
        name = PATTERN_NAMES[g % len(PATTERN_NAMES)]
        rng = np.random.default_rng([SEED, g])
        dests = np.asarray(codes, dtype=np.int64) % 90
        row = ROW_PATTERNS[name](dests, rng) if len(dests) else None
        if row is None:                                          # the pattern needs entries this list has not
            name, row = "uniform", _uniform(dests, rng)
        q[g] = row
        pattern.append(name)
    _cache["in"] = dict(boards=boards, meta=meta, lists=lists, q=q, pattern=pattern, longest=longest)
    return _cache["in"]


def philox_words(n=N_GAMES, seed=SEED, first_game_id=0, ply=0):
    """[n][4] the env kernel's Philox block of every game's ply (ply: a number or one per game)"""
    key = (n, seed, first_game_id, tuple(np.broadcast_to(ply, n).tolist()))
    if key not in _cache:
        plies = np.broadcast_to(ply, n)
        _cache[key] = np.array([xo.philox([int(plies[g]), 0, first_game_id + g, 0], [seed & 0xFFFFFFFF, seed >> 32]) for g in range(n)],
                               dtype=np.uint64)
    return _cache[key]


def expected(T, eps=0.0, q_view=False):
    """the reference on the shared inputs -> dict(idx, action (-1 without a move), explored, undecided), arrays over the games"""
    key = ("want", T, eps, q_view)
    if key in _cache:
        return _cache[key]
    inp, R = inputs(), philox_words()
    eps_u32 = int(min(max(float(eps), 0.0) * 4294967296.0, 4294967295.0))
    idx, act = np.full(N_GAMES, -1), np.full(N_GAMES, -1)
    expl, und = np.zeros(N_GAMES, np.int64), np.zeros(N_GAMES, bool)
    for g, codes in enumerate(inp["lists"]):
        if len(codes) == 0:
            continue
        swap = bool(q_view) and int(inp["meta"][g, 1]) == 1
        idx[g], expl[g], und[g] = bz.step(inp["q"][g], codes, T, R[g], eps_u32, swap)
        act[g] = int(codes[idx[g]])
    _cache[key] = dict(idx=idx, action=act, explored=expl, undecided=und)
    return _cache[key]


def candidate_vectors(q_view=False):
    """the games' candidate values v (float32, NaN -> -inf), padded with -inf to [n][128], and the list lengths"""
    inp = inputs()
    V = np.full((N_GAMES, 128), -np.inf, F32)
    n_of = np.zeros(N_GAMES, np.int64)
    for g, codes in enumerate(inp["lists"]):
        if len(codes):
            V[g, :len(codes)] = bz.values(inp["q"][g], codes, bool(q_view) and int(inp["meta"][g, 1]) == 1)
        n_of[g] = len(codes)
    return V, n_of
