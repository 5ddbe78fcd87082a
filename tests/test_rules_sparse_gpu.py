"""The rules kernels on positions random play never reaches — `pytest -m gpu`.

(1) FIXTURES.  tests/golden/ref_sparse.npz / ref_sparse_mat.npz (the unmodified reference engine under steering: bare endgames, far-rank
    soldiers, fallen generals, a side without a piece) through legal_moves, step, valid_matrix, rule_matrix and get_winner, each
    position loaded twice: with its true scores (META_TRACKED: reward, game-over and winner from the scores) and with both scores
    shifted by one soldier (untracked: from evaluate_board_wave / board_status_wave).  Lists, captures and boards must not depend on
    the load; reward, terminated, done and winner are the oracle's on the reference's after-state.
(2) GENERATED BOARDS, HIP == oracle bit for bit, seeded, per class (boards compared / batches of 16384):
      (a) legal-looking endgames, 1-6 pieces a side on squares their type can stand on          114 688
      (b) line stress: a chariot or cannon on every row / column index with every set of 0-3
          other pieces on its line, and the full line; once bare, once with clutter elsewhere    162 000
      (c) arbitrary placements of 0-16 pieces a side (generals anywhere, several generals, ...)  114 688
      (d) no piece of the side to move, and the empty board                                      114 688
    For every board: legal_moves(0), legal_moves(1) and the counts; one selfplay_step without Q (the move is the oracle's Philox
    pick; n_moves, reward, done, terminated, winner, scores, the board and meta after the move or the reset, and the episode
    records with their no-action mark); one selfplay_step with a Q row whose maximum sits on the last listed move's target (the
    first move onto that square wins).
(3) SEARCH.  search_values(1), (2) against tests/search_ref.py on every fixture position and on 2 000 boards of class (a); depth 3
    on 100 fixture positions with at most 6 pieces in all.
(4) THE 16-PIECE LIMIT.  xq_env_set_state and xq_replay_push_host refuse a 17th piece of one colour; sixteen chariots a side still
    match the oracle list for list; a list longer than kMaxMoves = 128 is the oracle's first 128 moves, count 128.

(5) WHOLE GAMES FROM SPARSE STARTS.  One arena (search-2 against random play, 64 pairs, no opening) and one versus collect loop (random
    opponent, 8 collects of 64 games), both started from class (a) boards with both generals, loaded through set_state into the
    arena's / the trainer's env (odd games with scores that do not explain the material: the board-scan path), and replayed ply by
    ply on the CPU as tests/test_search_gpu.py and tests/test_versus_gpu.py do: every action, the arena's records and final states, the
    versus boards, meta, ring slots, episode records and outcome counters.

Measured on one MI355X: sections (1)-(4) (14 tests) take 12.7 s; each generated class 1.8 - 2.7 s, most of it generating the boards
and the CPU oracle.  The figure does not include section (5).
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

import search_ref as sr
import xqoracle as xo
from sparse_boards import gen_arbitrary, gen_endgames, gen_line_stress

pytestmark = pytest.mark.gpu

BATCH = 16384
SOLDIER = 10                                            # one piece value: the shift that takes a load off the tracked path
INT32_MIN = np.iinfo(np.int32).min


# ------------------------------------------------------------------------------------------------ the oracle over a batch
BOARD_DT = np.dtype({"names": ["sq", "moveCount", "currentPlayer", "redScore", "blackScore"],
                     "formats": [("u1", (90,)), "<i4", "<i4", "<i4", "<i4"], "offsets": [0, 92, 96, 100, 104], "itemsize": 108})
assert C.sizeof(xo.Board) == BOARD_DT.itemsize


class OracleBatch:
    """xqoracle over n boards held in one array (ctypes views, no per-board copies)."""

    def __init__(self, boards, meta):
        self.n = len(boards)
        self.a = np.zeros(self.n, dtype=BOARD_DT)
        self.a["sq"] = boards
        for k, name in enumerate(("moveCount", "currentPlayer", "redScore", "blackScore")):
            self.a[name] = meta[:, k]

    def _views(self, a):
        return (xo.Board * self.n).from_buffer(a)

    def lists(self, colour):
        """-> (codes [n][128] zero-padded, counts clipped to 128, raw counts); colour -1 = the side to move"""
        L, arr = xo.lib(), self._views(self.a)
        codes = np.zeros((self.n, xo.MAX_MOVES), dtype=np.uint16)
        cv = ((C.c_uint16 * xo.MAX_MOVES) * self.n).from_buffer(codes)
        raw = np.zeros(self.n, dtype=np.int32)
        pl = self.a["currentPlayer"] if colour < 0 else np.full(self.n, colour)
        f = L.xqo_all_valid_actions
        for i in range(self.n):
            raw[i] = f(arr[i], int(pl[i]), cv[i])
        return codes, np.minimum(raw, xo.MAX_MOVES), raw

    def selfplay(self, q, seed, plies):
        """One oracle ply per board (game id = index) on a COPY -> (dict of result arrays, boards after, meta after).  A side without a
        move: the reward is evaluateBoard of the untouched board, as the device reports it."""
        L = xo.lib()
        a = self.a.copy()
        arr = self._views(a)
        out = xo.StepOut()
        names = ("action", "n_moves", "reward", "done", "terminated", "winner", "move_count", "red_score", "black_score")
        res = {k: np.zeros(self.n, dtype=np.int64) for k in names}
        qp = None
        step, ev = L.xqo_selfplay_step, L.xqo_evaluate_board
        ref = C.byref(out)
        for i in range(self.n):
            if q is not None:
                qp = q[i].ctypes.data_as(C.POINTER(C.c_float))
            b = arr[i]
            player, mc = b.currentPlayer, b.moveCount
            reward0 = ev(b, player, mc)
            step(b, qp, seed, i, int(plies[i]), 0, ref)
            row = (out.action_code, out.n_moves, out.reward if out.action_code >= 0 else reward0, out.done, out.terminated,
                   out.winner, out.moveCount, out.redScore, out.blackScore)
            for k, v in zip(names, row):
                res[k][i] = v
        meta = np.stack([a[k] for k in ("moveCount", "currentPlayer", "redScore", "blackScore")], axis=1)
        return res, a["sq"].copy(), meta


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} boards differ, first at {int(bad[0])}: got {got[bad[0]]!r} want {want[bad[0]]!r}")


# ------------------------------------------------------------------------------------------------ fixtures of the module
@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0, "no HIP device visible"
    return m


@pytest.fixture(scope="module")
def sparse(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_sparse.npz"))


def _meta(t, shift=0):
    return np.stack([t["moveCount"], t["player"], t["redScore"] + shift, t["blackScore"] + shift], axis=1).astype(np.int32)


def _ragged(t, key, i):
    return t[key][t[key + "_off"][i]:t[key + "_off"][i + 1]]


# ------------------------------------------------------------------------------------------------ (1) fixtures
@pytest.mark.parametrize("shift", [0, SOLDIER], ids=["tracked", "untracked"])
def test_legal_moves_match_sparse_fixture(xq, sparse, shift):
    n = len(sparse["moveCount"])
    env = xq.VecEnv(n)
    env.set_state(sparse["board"], _meta(sparse, shift))
    for colour, key in ((0, "red"), (1, "black")):
        codes, counts = env.legal_moves(colour)
        _same(counts, np.diff(sparse[key + "_off"]), key + " counts")
        for i in range(n):
            assert np.array_equal(codes[i, :counts[i]], _ragged(sparse, key, i)), (key, i)
            assert not codes[i, counts[i]:].any(), (key, i)
    codes, counts = env.legal_moves(-1)
    for i in range(n):
        key = "red" if sparse["player"][i] == 0 else "black"
        assert np.array_equal(codes[i, :counts[i]], _ragged(sparse, key, i)), i
    _same(env.get_winner(), sparse["winner"], "getWinner")
    env.close()


@pytest.mark.parametrize("shift", [0, SOLDIER], ids=["tracked", "untracked"])
def test_step_matches_sparse_fixture(xq, sparse, shift):
    """movePiece with the recorded attempts; the state after it is the REFERENCE's (after_board / after_meta), the same for both
    loads but for the shifted scores; reward, terminated, done and winner are the oracle's on that state."""
    n = len(sparse["moveCount"])
    L = xo.lib()
    env = xq.VecEnv(n)
    env.set_state(sparse["board"], _meta(sparse, shift))
    mv = sparse["move"].astype(np.int64)
    inb = ((mv >= 0).all(axis=1)) & (mv[:, 0] < 10) & (mv[:, 2] < 10) & (mv[:, 1] < 9) & (mv[:, 3] < 9)
    actions = np.where(inb, (mv[:, 0] * 9 + mv[:, 1]) * 90 + mv[:, 2] * 9 + mv[:, 3], -1).astype(np.int32)
    res = env.step(actions, auto_reset=False)
    boards, meta = env.get_state()
    _same(res["valid"], sparse["valid"], "valid")
    _same(res["captured"], sparse["captured"], "captured")
    _same(boards, sparse["after_board"], "board after the attempt")
    want_meta = sparse["after_meta"] + np.array([0, 0, shift, shift])
    _same(meta, want_meta, "meta after the attempt")
    for i in range(n):
        b = xo.board_from(sparse["after_board"][i], *(int(x) for x in want_meta[i]))
        mover = int(sparse["player"][i])
        over = L.xqo_check_game_over(C.byref(b))
        assert res["reward"][i] == L.xqo_evaluate_board(C.byref(b), mover, b.moveCount), i
        assert res["terminated"][i] == over, i
        assert res["done"][i] == int(over or b.moveCount + 1 >= 200), i
        assert res["winner"][i] == (L.xqo_get_winner(C.byref(b)) if over else 2), i
        assert (res["move_count"][i], res["red_score"][i], res["black_score"][i]) == (b.moveCount, b.redScore, b.blackScore), i
    env.close()


def test_matrices_match_sparse_fixture(xq, golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_sparse_mat.npz"))
    n = len(g["board"])
    env = xq.VecEnv(n)
    env.set_state(g["board"])
    for i in range(n):
        assert np.array_equal(env.valid_matrix(i), np.unpackbits(g["valid_bits"][i])[:8100]), i
        assert np.array_equal(env.rule_matrix(i), np.unpackbits(g["rule_bits"][i])[:7 * 8100].reshape(7, 8100)), i
    want = [xo.lib().xqo_get_winner(C.byref(xo.board_from(b))) for b in g["board"]]
    _same(env.get_winner(), want, "getWinner")
    env.close()


# ------------------------------------------------------------------------------------------------ (2) generated boards
def compare_class(xq, boards, meta, seed):
    """Every comparison of section (2) of the module docstring over one class -> boards compared."""
    env = xq.VecEnv(BATCH, seed=seed)
    plies = np.zeros(BATCH, dtype=np.int64)                 # the per-slot Philox counter survives set_state
    n_noaction = 0
    for lo in range(0, len(boards), BATCH):
        bb, mm = boards[lo:lo + BATCH], meta[lo:lo + BATCH]
        m = len(bb)
        ob = OracleBatch(bb, mm)
        env.set_state(bb, mm)
        for colour in (0, 1):
            codes, counts = env.legal_moves(colour)
            want_codes, want_counts, _ = ob.lists(colour)
            _same(counts[:m], want_counts, f"batch {lo} colour {colour} counts")
            _same(codes[:m], want_codes, f"batch {lo} colour {colour} lists")
        mover_codes, mover_counts, _ = ob.lists(-1)
        for q_step in (False, True):
            q = None
            if q_step:
                env.set_state(bb, mm)
                q = np.full((BATCH, 90), -0.5, dtype=np.float32)
                has = mover_counts > 0
                last_to = mover_codes[np.arange(m), np.maximum(mover_counts - 1, 0)] % 90
                q[np.nonzero(has)[0], last_to[has]] = 0.25
                first = np.array([next((int(c) for c in mover_codes[i, :mover_counts[i]] if int(c) % 90 == last_to[i]), -1)
                                  for i in range(m)])
            env.drain_episodes(4 * BATCH)
            res = env.selfplay_step(q, 0.0)[:m]
            want, want_boards, want_meta = ob.selfplay(q, seed, plies)
            for k, v in want.items():
                _same(res[k].astype(np.int64), v, f"batch {lo} q={q_step} {k}")
            if q_step:
                _same(res["action"].astype(np.int64), first, f"batch {lo}: the first move onto the best square")
                assert not res["explored"].any()
            got_boards, got_meta = env.get_state(0, m)
            _same(got_boards, want_boards, f"batch {lo} q={q_step} board after the ply")
            _same(got_meta, want_meta, f"batch {lo} q={q_step} meta after the ply")
            rec, _ = env.drain_episodes(4 * BATCH)
            rec = rec[rec["game_id"] < m]                   # (a short last batch leaves older games in the slots behind it)
            ended = np.nonzero(want["terminated"] != 0)[0]
            have = sorted(zip(rec["game_id"].tolist(), rec["red_score"].tolist(), rec["black_score"].tolist(),
                              rec["move_count"].tolist(), rec["winner"].tolist(), rec["reserved"].tolist()))
            assert have == sorted((int(g), int(want["red_score"][g]), int(want["black_score"][g]), int(want["move_count"][g]),
                                   int(want["winner"][g]), int(want["action"][g] < 0)) for g in ended), f"batch {lo} episode records"
            n_noaction += int((want["action"] < 0).sum())
            plies[:m] += want["action"] >= 0
    env.close()
    return len(boards), n_noaction


def test_generated_endgames_match_oracle(xq):
    n, n_noaction = compare_class(xq, *gen_endgames(7 * BATCH, 0xE17D), seed=101)
    assert n >= 100000 and n_noaction > 0


def test_generated_line_stress_matches_oracle(xq):
    n, _ = compare_class(xq, *gen_line_stress(0x11E5), seed=102)
    assert n >= 100000


def test_generated_arbitrary_placements_match_oracle(xq):
    n, _ = compare_class(xq, *gen_arbitrary(7 * BATCH, 0xA2B1), seed=103)
    assert n >= 100000


def test_generated_boards_without_a_piece_to_move_match_oracle(xq):
    boards, meta = gen_arbitrary(7 * BATCH, 0xD00D, empty_mover=True)
    n, n_noaction = compare_class(xq, boards, meta, seed=104)
    assert n >= 100000 and n_noaction == 2 * n               # both plies of every board end the episode without an action


# ------------------------------------------------------------------------------------------------ (3) search
def check_search(xq, boards, meta, depth):
    env = xq.VecEnv(len(boards))
    env.set_state(boards, meta)
    values, counts, best = env.search_values(depth)
    env.close()
    for i in range(len(boards)):
        b = sr.position(boards[i], int(meta[i][1]), *[int(x) for x in meta[i][[0, 2, 3]]])
        codes, vals = sr.root_values(b, int(meta[i][1]), depth)
        n = len(codes)
        assert counts[i] == n, i
        assert np.array_equal(values[i, :n], np.asarray(vals, dtype=np.int64)), (i, depth)
        assert np.all(values[i, n:] == INT32_MIN), i
        assert best[i] == (int(np.argmax(vals)) if n else -1), i


@pytest.mark.parametrize("depth", [1, 2])
def test_search_on_sparse_positions(xq, sparse, depth):
    check_search(xq, sparse["board"], _meta(sparse), depth)
    check_search(xq, *gen_endgames(2000, 0x5EA2), depth)


def test_search_depth3_on_sparse_positions(xq, sparse):
    """Subtrees in which a general falls and the line continues: 100 fixture positions with at most 6 pieces on the board."""
    few = np.nonzero((sparse["board"] != 0).sum(axis=1) <= 6)[0]
    few = few[(np.diff(sparse["red_off"])[few] > 0) | (np.diff(sparse["black_off"])[few] > 0)][:100]
    assert len(few) == 100
    check_search(xq, sparse["board"][few], _meta(sparse)[few], 3)


# ------------------------------------------------------------------------------------------------ (4) the 16-piece limit
def test_more_than_16_pieces_of_one_colour_are_refused(xq):
    ok = np.zeros(90, dtype=np.uint8)
    ok[:16] = 5                                              # sixteen red chariots
    ok[74:90] = 12                                           # sixteen black ones
    bad = ok.copy()
    bad[40] = 14                                             # a seventeenth black piece
    env = xq.VecEnv(3)
    before = env.get_state()
    for boards in (np.stack([ok, bad, ok]), np.stack([bad[::-1] % 8, ok, ok])):       # (the second: seventeen RED pieces)
        with pytest.raises(xq._capi.XqError) as e:
            env.set_state(boards)
        assert e.value.code == 1                             # XQ_ERR_INVALID_ARGUMENT
        after = env.get_state()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # nothing was written
    env.set_state(np.stack([ok, ok, ok]))
    env.close()
    rp = xq.ReplayBuffer(8)
    for s, s2 in ((bad, ok), (ok, bad)):
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(np.stack([ok, s]), [1, 2], [0.0, 0.0], [0, 0], np.stack([ok, s2]))
        assert e.value.code == 1
        assert rp.stats()[0] == 0                            # nothing was pushed
    rp.push(np.stack([ok, ok]), [1, 2], [0.0, 0.0], [0, 0], np.stack([ok, ok]))
    assert rp.stats()[0] == 2
    rp.close()


def test_sixteen_pieces_of_any_type_and_the_list_cap(xq):
    """A full 16-entry piece table of one type (chariots, cannons, horses, soldiers on any rank, generals) matches the oracle list
    for list.  Where a side has MORE than kMaxMoves = 128 moves the agreed behaviour is: the list is the first 128 moves in canonical
    order and the count is 128 — the oracle's xqo_all_valid_actions returns the true count and fills 128 entries, the kernel clips
    each run once; a selfplay_step picks among those 128."""
    rnd = random.Random(16)
    boards = []
    for t in (5, 6, 4, 7, 1, 2, 3):
        for _ in range(64):
            sq = rnd.sample(range(90), 32)
            b = np.zeros(90, dtype=np.uint8)
            b[sq[:16]] = t
            b[sq[16:]] = rnd.choice((t + 7, 12, 14))
            boards.append(b)
    for k in range(64):                                      # sixteen chariots against one piece: far more than 128 moves
        b = np.zeros(90, dtype=np.uint8)
        b[rnd.sample(range(90), 16)] = 5 if k % 2 == 0 else 12
        empty = np.nonzero(b == 0)[0]
        b[int(rnd.choice(empty))] = 8 if k % 2 == 0 else 1
        boards.append(b)
    boards = np.array(boards)
    meta = np.zeros((len(boards), 4), dtype=np.int32)
    meta[:, 1] = (boards[:, :] == 12).sum(axis=1) == 16      # the sixteen-chariot side moves in the last group
    ob = OracleBatch(boards, meta)
    env = xq.VecEnv(len(boards), seed=7)
    env.set_state(boards, meta)
    n_over = 0
    for colour in (0, 1):
        codes, counts = env.legal_moves(colour)
        want_codes, want_counts, raw = ob.lists(colour)
        _same(counts, want_counts, "counts")
        _same(codes, want_codes, "lists")
        n_over += int((raw > 128).sum())
        assert counts.max() <= 128
    assert n_over >= 32                                      # the cap was really exceeded
    res = env.selfplay_step(None)
    want, want_boards, _ = ob.selfplay(None, 7, np.zeros(len(boards), dtype=np.int64))
    _same(res["action"].astype(np.int64), want["action"], "the pick among the first 128")
    _same(res["n_moves"].astype(np.int64), want["n_moves"], "n_moves")
    _same(env.get_state()[0], want_boards, "board after the ply")
    env.close()


# ------------------------------------------------------------------------------------------------ (5) whole games from sparse starts
def sparse_starts(n, seed, move_count=None):
    """n class (a) boards on which both generals stand; odd ones get scores 0 / 0 (untracked), even ones scores that explain the
    material.  move_count None keeps the generated one."""
    boards, meta = gen_endgames(4 * n, seed)
    ok = np.nonzero((boards == 1).any(axis=1) & (boards == 8).any(axis=1))[0][:n]
    assert len(ok) == n
    boards, meta = boards[ok], meta[ok]
    tracked = np.arange(n) % 2 == 0
    value = np.array([0, 1000, 20, 20, 40, 90, 45, 10] + [1000, 20, 20, 40, 90, 45, 10])
    mat_red = (value[boards] * (boards <= 7)).sum(axis=1)
    mat_black = (value[boards] * (boards >= 8)).sum(axis=1)
    meta[:, 2] = np.where(tracked, 1480 - mat_black, 0)
    meta[:, 3] = np.where(tracked, 1480 - mat_red, 0)
    if move_count is not None:
        meta[:, 0] = move_count
    return boards, meta


def test_arena_from_sparse_starts_replays_on_cpu(xq):
    """Search-2 (eps 0.1) against random play, 64 pairs, opening 0.  The arena's games are loaded through its own env (xq_arena_env ->
    set_state after a reset): Red to move, move count 0, twins on the same board."""
    from cn_chess_ai_amd.arena import Arena, Search
    from test_arena_gpu import check_records
    from test_search_gpu import SearchReplay
    P, seed, depth, eps = 64, 31, 2, 0.1
    boards, meta = sparse_starts(P, 0xA4E7A, move_count=0)
    meta[:, 1] = 0
    boards, meta = np.concatenate([boards, boards]), np.concatenate([meta, meta])
    ar = Arena(P, seed=seed, opening_plies=0)
    ar.env.set_state(boards, meta)
    rp = SearchReplay(P, seed, 0, 0, depth, eps)
    rp.boards = [xo.board_from(boards[g], *(int(x) for x in meta[g])) for g in range(2 * P)]
    live = np.ones(2 * P, bool)
    ply = n_search = 0
    causes = set()
    while live.any():
        assert ply < 200
        ar.run(Search(depth, eps), None, 0.0, 0.0, max_plies=1)
        res = ar.last_step()
        for g in np.nonzero(live)[0]:
            g = int(g)
            act = rp.expected(g, ply, None)
            assert int(res[g]["action"]) == act, (g, ply, int(res[g]["action"]), act)
            n_search += (ply % 2 == 0) == (g < P)
            if rp.play(g, ply, act):
                live[g] = False
                causes.add(rp.rec[g][0])
        ply += 1
        assert ar.live() == int(live.sum())
    rec = check_records(ar, rp)
    ar.close()
    assert n_search > 100 and xq._capi.ARENA_GENERAL_CAPTURED in causes
    assert np.sum(rec["a_result"] > 0) > np.sum(rec["a_result"] < 0)


def test_versus_collects_from_sparse_starts_replay_on_cpu(xq):
    """tests/test_versus_gpu.py's replay of the collect loop (random opponent, 8 collects + updates of 64 games) with the trainer's env
    loaded from sparse boards instead of the start position: games end by capture, by a side without a move and by the move cap within
    the run, and start again from the start position."""
    import versus_ref as vr
    from test_dqn_gpu import REF_NET
    from test_versus_gpu import config, opponent, q_rows
    n, cap, mb, iters, seed, first, lr = 64, 512, 48, 8, 0x5A75, 3, 0.01
    t = xq.Trainer(config(xq, n, cap, mb, seed, first, lr=lr))
    t.dqn.set_params(*xo.init_weights(REF_NET, 21))
    arg, opp, _ = opponent(xq, "random")
    t.set_opponent(arg)
    scratch = xq.VecEnv(n, seed=seed, first_game_id=first)
    learner = xq.DQN(REF_NET, lr, 0.99, seed=1)
    boards, meta = sparse_starts(n, 0x7E25A, move_count=np.array([150 + (g * 7) % 50 for g in range(n)]))   # the cap ends some games
    t.env.set_state(boards, meta)
    games = [vr.Game(first + g, board=xo.board_from(boards[g], *(int(x) for x in meta[g]))) for g in range(n)]
    results, episodes = [], []
    for it in range(iters):
        w, b = t.dqn.get_params()
        learner.set_params(w, b)
        c = vr.Collect(seed, 0.1, opp)
        want = c.run(games, q_rows(xq, scratch, learner))
        results += c.results
        episodes += c.episodes
        t.collect()
        got_boards, got_meta = t.env.get_state()
        for g, game in enumerate(games):
            assert np.array_equal(got_boards[g], game.b.squares()), (it, g)
            assert list(got_meta[g]) == [game.b.moveCount, game.b.currentPlayer, game.b.redScore, game.b.blackScore], (it, g)
            s, a, r, dn, s2 = t.replay.get((it * n + g) % cap)
            ws, wa, wr, wd, ws2 = want[g]
            assert np.array_equal(s, ws) and np.array_equal(s2, ws2) and (a, r, dn) == (wa, float(wr), wd), (it, g)
        t.learn_grads()
        t.learn_apply(1)
    got = t.versus_results()
    res = np.array([r for _, r in results])
    assert (got["wins"], got["draws"], got["losses"], got["games"]) == \
        (int((res == 1).sum()), int((res == 0).sum()), int((res == -1).sum()), len(res))
    rec, _ = t.env.drain_episodes()
    have = sorted((int(e["game_id"]), int(e["episode"]), int(e["red_score"]), int(e["black_score"]), int(e["move_count"]),
                   int(e["winner"]), int(e["reserved"])) for e in rec)
    assert have == sorted(episodes)
    assert (res == 0).any() and (res != 0).any()            # games did end inside the run, by the cap and otherwise
    t.close(); scratch.close(); learner.close()
