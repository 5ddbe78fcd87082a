"""Search player on the device (DESIGN.md §4 "Search player"): xq_env_search value for value against tests/search_ref.py, arenas with a
search side replayed ply by ply on the CPU, exact self-play symmetry, strength, a borrowed trainer left bit-identical, full size, and
the C ABI's argument checks."""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest

import cn_chess_ai_amd as xq
from cn_chess_ai_amd import _capi
from cn_chess_ai_amd.arena import Arena, Search
import search_ref as sr
import xqoracle as xo

from test_arena_gpu import check_records, ref_net, trainer_run
from test_arena_cpu import build_example
from test_search_cpu import build_search_facade_probe

pytestmark = pytest.mark.gpu
INT32_MIN = np.iinfo(np.int32).min


@pytest.fixture(scope="module", autouse=True)
def device():
    if _capi.device_count() < 1:
        pytest.skip("no HIP device")
    _capi.call("xq_set_device", 0)


def golden(golden_dir, name):
    t = np.load(os.path.join(golden_dir, name))
    meta = np.stack([t["moveCount"], t["player"], t["redScore"], t["blackScore"]], axis=1).astype(np.int32)
    return t["board"], meta


def check_against_restatement(boards, meta, depth):
    env = xq.VecEnv(len(boards))
    env.set_state(boards, meta)
    values, counts, best = env.search_values(depth)
    env.close()
    for i in range(len(boards)):
        b = sr.position(boards[i], *[int(x) for x in meta[i]])
        codes, vals = sr.root_values(b, int(meta[i][1]), depth)
        n = len(codes)
        assert counts[i] == n, i
        assert np.array_equal(values[i, :n], np.asarray(vals, dtype=np.int64)), (i, depth)
        assert np.all(values[i, n:] == INT32_MIN), i
        assert best[i] == (int(np.argmax(vals)) if n else -1), i


@pytest.mark.parametrize("depth", [1, 2])
def test_env_search_matches_restatement(golden_dir, depth):
    for name in ("ref_trace.npz", "ref_bigmoves.npz"):
        check_against_restatement(*golden(golden_dir, name), depth)


def test_env_search_depth3_matches_restatement(golden_dir):
    boards, meta = golden(golden_dir, "ref_trace.npz")
    pick = np.arange(0, len(boards), 25)                       # 142 positions spread over the trace
    big_b, big_m = golden(golden_dir, "ref_bigmoves.npz")      # and every bigmoves position
    check_against_restatement(np.concatenate([boards[pick], big_b]), np.concatenate([meta[pick], big_m]), 3)


def test_env_search_rejects_other_depths():
    env = xq.VecEnv(2)
    for bad in (0, 4):
        with pytest.raises(xq.XqError):
            env.search_values(bad)
    env.close()


class SearchReplay:
    """An arena with a search player A replayed on the CPU: the opening and the random player as in test_arena_gpu.OracleArena, the search
    with search_ref.arena_pick; a network player B's moves are taken from the device trace (checked by tests/test_arena_gpu.py)."""

    def __init__(self, pairs, seed, first_id, opening, depth, eps):
        self.P, self.seed, self.first, self.opening, self.depth, self.eps = pairs, seed, first_id, opening, depth, eps
        self.boards = [xo.new_board() for _ in range(2 * pairs)]
        self.rec = [None] * (2 * pairs)
        self.final = [None] * (2 * pairs)

    def expected(self, g, ply, b_net_action):
        """-> the action code game g plays at this ply (-1: no legal move)"""
        b = self.boards[g]
        side = b.currentPlayer
        codes, _ = xo.all_valid_actions(b, side)
        if len(codes) == 0:
            return -1
        if ply < self.opening:
            r = xo.philox([ply, 0, self.first + g % self.P, 0], [self.seed & 0xFFFFFFFF, self.seed >> 32])
            return int(codes[r[1] % len(codes)])
        if (ply % 2 == 0) == (g < self.P):                       # A, the search, is to move
            return sr.arena_pick(b, side, self.depth, self.seed, self.first, g, self.P, ply, self.eps)
        if b_net_action is not None:
            return int(b_net_action)
        r = xo.philox([ply, 0, self.first + g, 0], [self.seed & 0xFFFFFFFF, self.seed >> 32])
        return int(codes[r[1] % len(codes)])

    def play(self, g, ply, code):
        """plays code (-1: none) on game g; -> True if the game ended"""
        b = self.boards[g]
        player = b.currentPlayer
        a_side = 0 if g < self.P else 1
        if code >= 0:
            f, t = divmod(code, 90)
            assert xo.lib().xqo_move_piece(C.byref(b), f // 9, f % 9, t // 9, t % 9) >= 0
            if not xo.lib().xqo_check_game_over(C.byref(b)):
                return False
            post = b.squares()
            if not (np.any(post == 1) and np.any(post == 8)):
                winner = xo.lib().xqo_get_winner(C.byref(b))
                cause, res = _capi.ARENA_GENERAL_CAPTURED, (1 if winner == a_side else -1)
            else:
                cause, res = _capi.ARENA_MOVE_CAP, 0
        else:
            cause, res = _capi.ARENA_NO_LEGAL_MOVE, (-1 if player == a_side else 1)
        winner = xo.lib().xqo_get_winner(C.byref(b))
        if ply < self.opening:
            cause, res = _capi.ARENA_OPENING, 0
        self.rec[g] = (cause, winner, res, 1 if g < self.P else 0, b.moveCount, b.redScore, b.blackScore)
        self.final[g] = (b.squares(), (b.moveCount, b.currentPlayer, b.redScore, b.blackScore))
        return True


def replay_arena(opponent, depth, P=64, seed=29, eps=0.1, opening=6):
    net = opponent
    ar = Arena(P, seed=seed, opening_plies=opening)
    rp = SearchReplay(P, seed, 0, opening, depth, eps)
    live = np.ones(2 * P, bool)
    ply = n_search = 0
    while live.any():
        assert ply < 200
        ar.run(Search(depth, eps), net, 0.0, 0.0, max_plies=1)
        res = ar.last_step()
        for g in np.nonzero(live)[0]:
            g = int(g)
            a_moves = (ply % 2 == 0) == (g < P)
            net_action = int(res[g]["action"]) if (net is not None and not a_moves and ply >= opening) else None
            act = rp.expected(g, ply, net_action)
            assert int(res[g]["action"]) == act, (g, ply, int(res[g]["action"]), act)
            n_search += a_moves and ply >= opening
            if rp.play(g, ply, act):
                live[g] = False
        ply += 1
        assert ar.live() == int(live.sum())
    rec = check_records(ar, rp)
    ar.close()
    return rec, n_search


@pytest.mark.parametrize("depth", [2, 3])
def test_search_against_random_replays_on_cpu(depth):
    rec, n_search = replay_arena(None, depth)
    assert n_search > 100
    assert np.sum(rec["a_result"] > 0) > np.sum(rec["a_result"] < 0)


def test_search_against_net_replays_on_cpu():
    d, _, _ = ref_net(51)
    rec, n_search = replay_arena(d, 2)
    assert n_search > 100
    d.close()


def test_search_against_itself_is_exactly_even():
    P = 512
    ar = Arena(P, seed=17)
    ar.run(Search(2), Search(2))
    rec = ar.results()
    assert ar.live() == 0
    assert np.all(rec["a_result"][:P] + rec["a_result"][P:] == 0)
    assert np.array_equal(rec["cause"][:P], rec["cause"][P:]) and np.array_equal(rec["plies"][:P], rec["plies"][P:])
    s = ar.summary()
    assert s["scored_games"] > 0 and s["score"] == 0.5, s
    ar.close()


def test_strength():
    P = 4096
    ar = Arena(P, seed=23)
    ar.run(Search(2), None)
    s_random = ar.summary()
    ar.reset(8)
    ar.run(Search(2), Search(1))
    s_d1 = ar.summary()
    print(f"search-2 vs random: {s_random}\nsearch-2 vs search-1: {s_d1}")
    assert s_random["score"] >= 0.9, s_random
    assert s_d1["ci95"][0] > 0.5, s_d1
    ar.close()


def trainer_run_against_search(k1, k2):
    """test_arena_gpu.trainer_run with the lent network playing Search(2) in between"""
    cfg = xq.TrainerConfig(n_games=512, layer_sizes=(1260, 128, 128, 8100), replay_capacity=1 << 14, minibatch=512,
                           td_net=_capi.TD_ONLINE_NET, collects_per_update=4, seed=0x5EED, first_game_id=0)
    t = xq.Trainer(cfg)
    t.dqn.set_l0_derive(True)
    t.step(k1)
    before = (t.counters(), t.dqn.qmax_stats(), t.dqn.qmax_guard())
    ar = Arena(256, seed=4)
    ar.run(t.dqn, Search(2), 0.05)
    assert ar.live() == 0
    ar.close()
    assert (t.counters(), t.dqn.qmax_stats(), t.dqn.qmax_guard()) == before
    t.step(k2)
    out = t.dqn.get_params(), t.counters(), t.dqn.qmax_stats()
    t.close()
    return out


def test_borrowed_trainer_network_is_untouched_by_a_search_arena():
    (w0, b0), c0, q0 = trainer_run(6, 6, False)
    (w1, b1), c1, q1 = trainer_run_against_search(6, 6)
    assert np.array_equal(w0, w1) and np.array_equal(b0, b1)
    assert c0 == c1 and q0 == q1


def test_full_size_search_against_random():
    P = 4096
    ar = Arena(P, seed=3)
    t0 = time.perf_counter()
    plies = ar.run(Search(2, 0.1), None)
    sec = time.perf_counter() - t0
    rec = ar.results()
    print(f"arena 8192 games search-2 vs random: {plies} plies in {sec * 1e3:.2f} ms; "
          f"causes {np.bincount(rec['cause'], minlength=5).tolist()}")
    assert plies <= 200 and ar.live() == 0 and np.all(rec["cause"] != _capi.ARENA_LIVE)
    assert np.all(rec["plies"] <= 200) and np.all(np.abs(rec["a_result"]) <= 1)
    assert np.all(rec["a_is_red"][:P] == 1) and np.all(rec["a_is_red"][P:] == 0)
    cap = rec["cause"] == _capi.ARENA_MOVE_CAP
    assert np.all(rec["plies"][cap] == 200) and np.all(rec["a_result"][cap] == 0)
    gen = rec["cause"] == _capi.ARENA_GENERAL_CAPTURED
    assert np.all(rec["a_result"][gen] != 0)
    assert np.all(rec["winner"][gen] == np.where(rec["a_result"][gen] > 0, 1 - rec["a_is_red"][gen], rec["a_is_red"][gen]))
    s = ar.summary()
    assert 0.0 <= s["score"] <= 1.0 and s["ci95"][0] <= s["score"] <= s["ci95"][1]
    with pytest.raises(xq.XqError):
        ar.run(Search(2), None)                                # finished: nothing left to play
    ar.close()


def test_invalid_players():
    ar = Arena(4)
    d = xq.DQN((1260, 32, 96), seed=1)
    P = _capi.ArenaPlayer
    bad = [P(7, None, 0, 0.0), P(_capi.PLAYER_SEARCH, None, 0, 0.0), P(_capi.PLAYER_SEARCH, None, 4, 0.0),
           P(_capi.PLAYER_SEARCH, None, 2, -0.5), P(_capi.PLAYER_NET, None, 0, 0.0), P(_capi.PLAYER_NET, d.handle, 0, 2.0)]
    n = C.c_int32()
    for p in bad:
        rc = _capi.load().xq_arena_run_players(ar.handle, C.byref(p), None, 1, C.byref(n))
        assert rc == 1, (p.kind, p.depth, p.eps)
        assert _capi.load().xq_last_error()
    assert ar.live() == 8                                       # nothing was played
    ar.close(), d.close()


def test_example_and_facade_play_the_search(tmp_path):
    P, seed = 64, 5
    ar = Arena(P, seed=seed)
    ar.run(Search(2, 0.1), None)
    ref = ar.summary()
    ar.close()
    ex = build_example()
    out = subprocess.run([ex, "search2", "random", str(P), "--seed", str(seed), "--eps-a", "0.1", "--json"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    js = json.loads(out.stdout.strip().splitlines()[-1])
    assert (js["wins"], js["draws"], js["losses"]) == (ref["wins"], ref["draws"], ref["losses"])
    out = subprocess.run([ex, "search1", "search3", "16", "--json"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    fp = build_search_facade_probe()
    out = subprocess.run([fp, str(P), str(seed), "2"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    js = json.loads(out.stdout.strip().splitlines()[-1])
    assert (js["wins"], js["draws"], js["losses"]) == (ref["wins"], ref["draws"], ref["losses"])
    assert js["net_games"] > 0 and js["start_count"] == 44 and 0 <= js["start_best"] < 44
