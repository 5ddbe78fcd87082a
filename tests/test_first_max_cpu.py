"""CPU checks of the arg-max rule and of the table that tests it on the device (tests/first_max.py, tests/argmax_edge_cases.py).

1. first_max.pick agrees exactly with both restatements of DQN::selectAction in the oracle (xqo_selfplay_step's greedy branch on a
   fp32 row, xqo_select_action on doubles) on every Q-row pattern over random-play positions and the positions with 65..77 moves.
2. Negative control: six wrong rules, each a Python variant of the loop, must each play another move than the rule on at least 5 % of
   the (position, pattern) pairs; a variant that moves no pick would mean the table cannot tell that rule apart.
3. The Double-DQN table: on the reference's own activations at least three base rows win across a batch, and the samples whose top
   two base values lie within CAND_MARGIN (they are left out on the device) stay under 2 % for every case, layout and seed.
"""
import ctypes as C
import os

import numpy as np
import pytest

import argmax_edge_cases as ac
import batch_ref as br
import first_max as fm
import xqoracle as xo
from test_batch_ref_cpu import oracle_positions

PICK_SEED = 0x5EED + 41
MAX_LEFT_OUT = 0.02


# ---- the positions of the pick tests (shared with tests/test_first_maximum_gpu.py) --------------------------------------------------------
_positions = {}


def pick_positions(golden_dir, n_random=256):
    """(boards [n][90], meta [n][4], legal lists) of n_random random-play positions after 25 plies and of every position of
    ref_bigmoves.npz (65..77 moves for the side to move in most of them: the second half of the 128-entry list)"""
    if n_random not in _positions:
        S, P, _ = oracle_positions(n_random, 25, PICK_SEED)
        meta = np.stack([np.full(n_random, 25), P, np.zeros(n_random), np.zeros(n_random)], axis=1).astype(np.int32)
        t = np.load(os.path.join(golden_dir, "ref_bigmoves.npz"))
        bm = np.stack([t["moveCount"], t["player"], t["redScore"], t["blackScore"]], axis=1).astype(np.int32)
        # a record's long list may be the other side's: positions once more with that side to move, those with a long list first, up to
        # 512 games in all
        other = bm.copy()
        other[:, 1] ^= 1
        cnt_other = [xo.all_valid_actions(xo.board_from(t["board"][i], *other[i]), int(other[i, 1]))[1] for i in range(len(bm))]
        long_other = sorted(range(len(bm)), key=lambda i: (cnt_other[i] <= 64, i))[:512 - n_random - len(bm)]
        boards = np.concatenate([S, t["board"].astype(np.uint8), t["board"][long_other].astype(np.uint8)])
        meta = np.concatenate([meta, bm, other[long_other]])
        lists = []
        for s, m in zip(boards, meta):
            codes, cnt = xo.all_valid_actions(xo.board_from(s, *m), int(m[1]))
            lists.append(codes[:cnt])
        assert sum(len(c) > 64 for c in lists) >= 100
        _positions[n_random] = (boards, meta, lists)
    return _positions[n_random]


def oracle_step(board, meta, q, game, seed=PICK_SEED):
    """xqo_selfplay_step at epsilon 0 on a copy of the position -> (StepOut, squares after the ply)"""
    b = xo.board_from(board, *meta)
    o = xo.selfplay_step(b, q, seed, game, 0, 0)
    return o, b.squares()


def test_pick_agrees_with_both_oracle_restatements_on_every_pattern(golden_dir):
    boards, meta, lists = pick_positions(golden_dir)
    L = xo.lib()
    applied = {}
    for name in ac.Q_PATTERNS:
        q, ok = ac.q_rows(name, lists)
        applied[name] = int(ok.sum())
        for g, codes in enumerate(lists):
            if len(codes) == 0:
                continue
            want = fm.pick(q[g], codes)
            o, _ = oracle_step(boards[g], meta[g], q[g], g)
            assert o.action_code == int(codes[want]) and not o.explored, (name, g)
            q64 = q[g].astype(np.float64)
            cc = np.ascontiguousarray(codes, dtype=np.uint16)
            got = L.xqo_select_action(q64.ctypes.data_as(C.POINTER(C.c_double)), 90, cc.ctypes.data_as(C.POINTER(C.c_uint16)),
                                      len(cc), 0x7fffffff, 0, 0x7fffffff, -1.0)
            assert got == want, (name, g)
    print("games a pattern applies to:", applied)
    # every pattern really lands somewhere.  A tie between entries at or above 64 needs two squares that no earlier entry reaches, which
    # only some of the long lists have: dozens of positions, where one would do to catch a kernel that handles the second half wrongly
    for name, cnt in applied.items():
        assert cnt >= (32 if name in ac.LONG_LIST_ONLY else 0.9 * len(lists)), (name, cnt)


# ---- the wrong rules --------------------------------------------------------------------------------------------------------------------------
NEG = float("-inf")


def _last_maximum(v):
    best, idx = NEG, 0
    for k, x in enumerate(v):
        if x > best or (x == best and x > NEG):
            best, idx = x, k
    return idx


def _greater_or_equal(v):
    best, idx = NEG, 0
    for k, x in enumerate(v):
        if x >= best:
            best, idx = x, k
    return idx


def _nan_wins(v):
    for k, x in enumerate(v):
        if x != x:
            return k
    return fm.first_max(v)


def _denormals_flushed(v):
    tiny = float(np.finfo(np.float32).tiny)
    return fm.first_max([0.0 if abs(x) < tiny else x for x in v])


def _second_half_on_a_tie(v):
    a = fm.first_max(v[:64])
    if len(v) <= 64:
        return a
    b = fm.first_max(v[64:])
    va, vb = (x if x == x else NEG for x in (v[a], v[64 + b]))
    return 64 + b if vb >= va else a


def _nothing_wins_gives_the_last(v):
    best, idx = NEG, len(v) - 1
    for k, x in enumerate(v):
        if x > best:
            best, idx = x, k
    return idx


WRONG_RULES = {"last_maximum": _last_maximum, "greater_or_equal": _greater_or_equal, "nan_wins": _nan_wins,
               "denormals_flushed": _denormals_flushed, "second_half_on_a_tie": _second_half_on_a_tie,
               "nothing_wins_gives_the_last": _nothing_wins_gives_the_last}


@pytest.fixture(scope="module")
def candidate_values(golden_dir):
    """the candidates' values q[code % 90] of every (position, pattern) pair the pattern applies to, and the rule's pick"""
    _, _, lists = pick_positions(golden_dir)
    out = []
    for name in ac.Q_PATTERNS:
        q, ok = ac.q_rows(name, lists)
        for g in np.nonzero(ok)[0]:
            v = [float(q[g, int(c) % 90]) for c in lists[g]]
            out.append((v, fm.first_max(v)))
    return out


@pytest.mark.parametrize("rule", list(WRONG_RULES))
def test_a_wrong_rule_moves_picks_on_the_table(candidate_values, rule):
    moved = sum(WRONG_RULES[rule](v) != want for v, want in candidate_values)
    print(f"{rule}: another move on {moved} of {len(candidate_values)} (position, pattern) pairs")
    assert moved >= 0.05 * len(candidate_values), (rule, moved, len(candidate_values))


# ---- the Double-DQN table -----------------------------------------------------------------------------------------------------------------------
def ddqn_batch(c):
    """(S, S2) of a case: S2 are random-play positions of the oracle (the shared 2048 of test_batch_ref_cpu), S the same rolled by one"""
    P = oracle_positions()[0]
    start = (c.seed * 97) % (len(P) - c.n)
    S2 = P[start:start + c.n]
    return np.roll(S2, 1, axis=0), S2


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def ddqn_params(c, layout, nonfinite=None):
    """float64 parameters of the online and the target net of a case: U(-0.05, 0.05) hidden layers with non-zero biases (layer 0
    scaled by L0_SCALE), the online head of argmax_edge_cases.online_head, the target head with zero weights and the decoding biases.
    Returns ((w, b, wt, bt), positions per base row, the row every sample must pick or None)."""
    nw, nb = xo.nn_counts(c.sizes)
    Hl, NO = c.sizes[-2], c.sizes[-1]
    out = []
    for k in (0, 1):
        w, _ = xo.init_weights(c.sizes, 21 + c.seed + 50 * k)
        w[:c.sizes[0] * c.sizes[1]] *= ac.L0_SCALE               # hidden activations of O(1) that change sign from position to position
        b = np.random.default_rng(121 + c.seed + 50 * k).uniform(-0.05, 0.05, size=nb)
        out += [w, b]
    # the base rows' biases centre their values over the batch (the reference's hidden activations have a large part that all
    # positions share, and one base row would win nearly everywhere): every row, and so every set of positions, decides many samples
    out[0][nw - NO * Hl:] = 0.0
    hid = br.Net(c.sizes, _f32(out[0]), _f32(out[1]), c.prec)
    a_last = hid.hidden(br.one_hot(ddqn_batch(c)[1]))[-1]
    Wb = ac.base_rows(Hl, c.seed)[0]
    Wb = br.bf16_round(Wb) if c.prec else _f32(Wb)
    W, b, _, lay, force = ac.online_head(layout, NO, Hl, c.seed, nonfinite, base_bias=-(a_last @ Wb.T).mean(axis=0))
    out[0][nw - NO * Hl:] = W.reshape(-1)
    out[1][nb - NO:] = b
    out[2][nw - NO * Hl:] = 0.0
    out[3][nb - NO:] = ac.target_bias(NO)
    return out, lay, force


def ddqn_expected(c, w32, b32, S2, lay, force):
    """From the online parameters as the device holds them (fp32 values): (expected a* per sample, left-out mask, winning base row).
    The winner is the first maximum in fp64 of the EIGHT base values (the operands of the case's precision), never of 8100 columns;
    a* is the lowest position of its set; a sample whose top two base values are closer than CAND_MARGIN is left out."""
    net = br.Net(c.sizes, w32, b32, c.prec)
    a_last = net.hidden(br.one_hot(S2))[-1]
    rows = [pos[0] for pos in lay]
    z = net.Bf[-1][rows] + a_last @ net.Wf[-1][rows].T
    assert np.isfinite(z).all()
    win = np.array([fm.first_max(r) for r in z])
    top = np.sort(z, axis=1)
    left_out = (top[:, -1] - top[:, -2]) < br.CAND_MARGIN[c.prec]
    want = np.array([min(lay[r]) for r in win])
    if force is not None:
        want[:], left_out[:] = force, False
    return want, left_out, win


DDQN_RUNS = [(c, lay, None) for c in ac.DDQN_CASES for lay in ac.layouts()] + \
            [(c, "sets_0_7", nf) for c in ac.DDQN_CASES[:1] + ac.DDQN_CASES[3:4] for nf in ac.NONFINITE]


@pytest.mark.parametrize("c,layout,nonfinite", DDQN_RUNS, ids=[f"{c.name}-{lay}-{nf}" for c, lay, nf in DDQN_RUNS])
def test_ddqn_table_spreads_its_winners_and_leaves_few_samples_out(c, layout, nonfinite):
    (w, b, _, _), lay, force = ddqn_params(c, layout, nonfinite)
    _, S2 = ddqn_batch(c)
    want, left_out, win = ddqn_expected(c, _f32(w), _f32(b), S2, lay, force)
    share = float(left_out.mean())
    print(f"{c.name} {layout} {nonfinite}: winners {np.bincount(win, minlength=ac.N_BASE).tolist()} left out {share:.4f}")
    assert len(np.unique(win)) >= 3
    assert np.bincount(win, minlength=ac.N_BASE).min() >= 10   # every set of positions decides samples, not only three of them
    assert share <= MAX_LEFT_OUT
    if layout == "zero_rows":                                   # the signed zeros really decide samples
        assert (win == 0).mean() > 0.1


def test_decoding_grid_separates_neighbouring_rows():
    """neighbouring rows of the target head differ by ~2.4e-4 gamma in y: far above the fp32 bar of 2e-6 on the decoding residual"""
    grid = ac.GAMMA * np.tanh(ac.target_bias(8100).astype(np.float32).astype(np.float64))
    assert np.diff(grid).min() > 2.0e-4
    k, res = ac.decode_astar(grid[[0, 17, 4101, 8099]].astype(np.float32), 8100)
    assert k.tolist() == [0, 17, 4101, 8099] and res.max() < 1e-7
