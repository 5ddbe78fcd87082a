"""Arena on the device (DESIGN.md §4 "Arena"): every ply, final board and record against oracle/xqoracle.py selfplay_step with the
arena's seat / stream rules; self-play symmetry; real nets against the fp64 oracle; borrowed handles left bit-identical; full size."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import cn_chess_ai_amd as xq
from cn_chess_ai_amd import _capi
from cn_chess_ai_amd.arena import Arena
import xqoracle as xo

from test_arena_cpu import build_example, build_facade_probe

pytestmark = pytest.mark.gpu
REF_TOPOLOGY = (1260, 256, 256, 8100)


@pytest.fixture(scope="module", autouse=True)
def device():
    if _capi.device_count() < 1:
        pytest.skip("no HIP device")
    _capi.call("xq_set_device", 0)


class OracleArena:
    """The arena's rules spelled out on the CPU oracle, one game at a time."""

    def __init__(self, pairs, seed, first_id, opening):
        self.P, self.seed, self.first, self.opening = pairs, seed, first_id, opening
        self.boards = [xo.new_board() for _ in range(2 * pairs)]
        self.rec = [None] * (2 * pairs)
        self.final = [None] * (2 * pairs)

    def a_moves(self, g, ply):
        return (ply % 2 == 0) == (g < self.P)

    def step(self, g, ply, q90, eps_a, eps_b):
        """-> action code played (-1 = no legal move)"""
        b = self.boards[g]
        pre, player = b.squares(), b.currentPlayer
        opening = ply < self.opening
        sid = self.first + (g % self.P if opening else g)
        eps = eps_a if self.a_moves(g, ply) else eps_b
        o = xo.selfplay_step(b, None if opening else q90, self.seed, sid, ply, xo.eps_to_u32(eps))
        if o.terminated:
            post = pre.copy()
            if o.action_code >= 0:
                f, t = divmod(o.action_code, 90)
                post[t], post[f] = post[f], 0
            a_side = 0 if g < self.P else 1
            if o.action_code < 0:
                cause, res = _capi.ARENA_NO_LEGAL_MOVE, (-1 if player == a_side else 1)
            elif not (np.any(post == 1) and np.any(post == 8)):
                cause, res = _capi.ARENA_GENERAL_CAPTURED, (1 if o.winner == a_side else -1)
            else:
                cause, res = _capi.ARENA_MOVE_CAP, 0
            if opening:
                cause, res = _capi.ARENA_OPENING, 0
            self.rec[g] = (cause, o.winner, res, 1 if g < self.P else 0, o.moveCount, o.redScore, o.blackScore)
            self.final[g] = (post, (o.moveCount, player ^ (1 if o.action_code >= 0 else 0), o.redScore, o.blackScore))
        return o.action_code, bool(o.terminated)


def check_records(arena, orc):
    rec = arena.results()
    for g in range(2 * orc.P):
        r = rec[g]
        got = (int(r["cause"]), int(r["winner"]), int(r["a_result"]), int(r["a_is_red"]), int(r["plies"]), int(r["red_score"]),
               int(r["black_score"]))
        assert got == orc.rec[g], (g, got, orc.rec[g])
    boards, meta = arena.env.get_state()
    for g in range(2 * orc.P):
        post, m = orc.final[g]
        assert np.array_equal(boards[g], post), g
        assert tuple(int(x) for x in meta[g]) == m, (g, tuple(meta[g]), m)
    return rec


def test_explicit_q_matches_oracle_ply_by_ply():
    import torch
    P, seed, first, opening, eps_a, eps_b = 48, 77, 1000, 6, 0.1, 0.3
    ar = Arena(P, seed=seed, first_game_id=first, opening_plies=opening)
    orc = OracleArena(P, seed, first, opening)
    rng = np.random.default_rng(3)
    live = np.ones(2 * P, bool)
    ply, keep = 0, []
    while live.any():
        assert ply < 200
        q = np.tanh(rng.standard_normal((2 * P, 96))).astype(np.float32)
        if ply == 9:
            q[:] = 0.25                                        # every candidate ties: the first legal action wins
        qd = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        keep.append(qd)
        ar.ply_q_dev(qd, 96, eps_a, eps_b)
        res = ar.last_step()
        for g in np.nonzero(live)[0]:
            act, term = orc.step(int(g), ply, q[g, :90], eps_a, eps_b)
            assert int(res[g]["action"]) == act, (g, ply)
            if term:
                live[g] = False
        ply += 1
        if ply == opening:                                     # twins played the same opening
            boards, meta = ar.env.get_state()
            assert np.array_equal(boards[:P], boards[P:]) and np.array_equal(meta[:P], meta[P:])
        assert ar.live() == int(live.sum())
    check_records(ar, orc)
    with pytest.raises(xq.XqError):                            # a ply after the arena has finished
        ar.ply_q_dev(keep[-1], 96, eps_a, eps_b)
    ar.close()


def test_random_vs_random_matches_oracle():
    P, seed, first = 256, 5, 0
    ar = Arena(P, seed=seed, first_game_id=first)
    plies = ar.run(None, None)
    assert plies <= 200 and ar.live() == 0
    orc = OracleArena(P, seed, first, 8)
    for g in range(2 * P):
        for ply in range(200):
            if orc.step(g, ply, None, 0.0, 0.0)[1]:
                break
    check_records(ar, orc)
    ar.close()


def ref_net(seed, stream=None, precision=None):
    d = xq.DQN(REF_TOPOLOGY, seed=1, stream=stream)
    w, b = xo.init_weights(REF_TOPOLOGY, seed)
    b = np.random.default_rng(seed + 100).uniform(-0.05, 0.05, size=b.shape)
    d.set_params(w, b)
    if precision is not None:
        d.set_precision(precision)
    return d, w, b


def test_self_evaluation_is_exactly_even_and_stream_independent():
    P = 512
    d, w, b = ref_net(11)
    ar = Arena(P, seed=9)
    ar.run(d, d)
    rec = ar.results()
    assert ar.live() == 0
    scored = rec["cause"][:P] != _capi.ARENA_OPENING
    assert np.all(rec["a_result"][:P] + rec["a_result"][P:] == 0)
    assert np.array_equal(rec["plies"][:P], rec["plies"][P:]) and np.array_equal(rec["cause"][:P], rec["cause"][P:])
    s = ar.summary()
    assert scored.any() and s["score"] == 0.5, s
    # two handles, identical parameters, each on a stream of its own
    d1 = xq.DQN(REF_TOPOLOGY, seed=2)
    d2 = xq.DQN(REF_TOPOLOGY, seed=3)
    d1.set_params(w, b), d2.set_params(w, b)
    assert d1.stream() != d2.stream()
    ar.reset(8)
    ar.run(d1, d2)
    assert np.array_equal(ar.results(), rec)
    for h in (ar, d, d1, d2):
        h.close()


@pytest.mark.parametrize("precision,tol", [(_capi.PRECISION_F32, 1e-5), (_capi.PRECISION_BF16, 1e-2)])
def test_real_nets_against_fp64_oracle(precision, tol):
    P, seed, eps_a, eps_b, opening = 8, 21, 0.15, 0.25, 4
    da, wa, ba = ref_net(31, precision=precision)
    db, wb, bb = ref_net(32, precision=precision)
    ar = Arena(P, seed=seed, opening_plies=opening)
    live = np.ones(2 * P, bool)
    n_greedy = n_explored = 0
    for ply in range(40):
        boards, meta = ar.env.get_state()
        ar.run(da, db, eps_a, eps_b, max_plies=1)
        res = ar.last_step()
        for g in np.nonzero(live)[0]:
            b = xo.board_from(boards[g], *[int(x) for x in meta[g]])
            codes, _ = xo.all_valid_actions(b, int(meta[g][1]))
            a = int(res[g]["action"])
            if len(codes) == 0:
                assert a == -1
            else:
                a_moves = (ply % 2 == 0) == (g < P)
                sid = (g % P) if ply < opening else g
                r = xo.philox([ply, 0, sid, 0], [seed & 0xFFFFFFFF, seed >> 32])
                explore = ply < opening or r[0] < xo.eps_to_u32(eps_a if a_moves else eps_b)
                if explore:
                    assert a == int(codes[r[1] % len(codes)]), (g, ply)
                    n_explored += 1
                else:
                    w, bi = (wa, ba) if a_moves else (wb, bb)
                    q = xo.nn_forward(REF_TOPOLOGY, w, bi, xo.state_repr(b))
                    best = max(q[c % 90] for c in codes)
                    assert abs(q[a % 90] - best) <= tol, (g, ply, q[a % 90], best)
                    assert a in [int(c) for c in codes]
                    n_greedy += 1
            if res[g]["terminated"]:
                live[g] = False
        if not live.any():
            break
    assert n_greedy > 100 and n_explored > 20
    for h in (ar, da, db):
        h.close()


def trainer_run(k1, k2, with_arena):
    cfg = xq.TrainerConfig(n_games=512, layer_sizes=(1260, 128, 128, 8100), replay_capacity=1 << 14, minibatch=512,
                           td_net=_capi.TD_ONLINE_NET, collects_per_update=4, seed=0x5EED, first_game_id=0)
    t = xq.Trainer(cfg)
    t.dqn.set_l0_derive(True)
    t.step(k1)
    if with_arena:
        before = (t.counters(), t.dqn.qmax_stats(), t.dqn.qmax_guard())
        ar = Arena(256, seed=4)
        ar.run(t.dqn, None, 0.05, 0.0)
        assert ar.live() == 0
        ar.close()
        assert (t.counters(), t.dqn.qmax_stats(), t.dqn.qmax_guard()) == before
    t.step(k2)
    out = t.dqn.get_params(), t.counters(), t.dqn.qmax_stats()
    t.close()
    return out


def test_borrowed_trainer_network_is_untouched():
    (w0, b0), c0, q0 = trainer_run(6, 6, False)
    (w1, b1), c1, q1 = trainer_run(6, 6, True)
    assert np.array_equal(w0, w1) and np.array_equal(b0, b1)
    assert c0 == c1 and q0 == q1


def test_full_size_against_random():
    import time
    P = 4096
    d = xq.DQN((1260, 128, 8100), seed=1)
    w, b = xo.init_weights((1260, 128, 8100), 7)
    d.set_params(w, b)
    ar = Arena(P, seed=3)
    ar.run(d, None)                                            # warm-up (workspaces)
    ar.reset(8)
    t0 = time.perf_counter()
    plies = ar.run(d, None)
    sec = time.perf_counter() - t0
    rec = ar.results()
    print(f"arena 8192 games 1260-128-8100 vs random: {plies} plies in {sec * 1e3:.2f} ms = {2 * P / sec:.0f} games/s, "
          f"{2 * P * plies / sec:.3e} game-plies/s; causes {np.bincount(rec['cause'], minlength=5).tolist()}")
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
        ar.run(d, None)                                        # finished: nothing left to play
    ar.close(), d.close()


def test_example_and_evaluate_against_match_python(tmp_path):
    sizes = (1260, 128, 8100)
    paths = []
    for k in (41, 42):
        d = xq.DQN(sizes, seed=1)
        w, b = xo.init_weights(sizes, k)
        d.set_params(w, b)
        p = tmp_path / f"m{k}.bin"
        d.saveModel(str(p))
        d.close()
        paths.append(str(p))
    P, seed = 200, 13
    da, db = xq.DQN(sizes, seed=1), xq.DQN(sizes, seed=1)
    da.loadModel(paths[0]), db.loadModel(paths[1])
    ar = Arena(P, seed=seed)
    ar.run(da, db)
    ref = ar.summary()
    ar.reset(8)
    ar.run(da, None)
    ref_random = ar.summary()

    def same(js, s):
        assert (js["wins"], js["draws"], js["losses"]) == (s["wins"], s["draws"], s["losses"])
        assert js["causes"] == [s["causes"][k] for k in ("live", "general_captured", "no_legal_move", "move_cap", "opening")]
        assert abs(js["score"] - s["score"]) < 1e-9 and abs(js["elo"] - s["elo"]) < 1e-6
        assert np.allclose(js["ci95"], s["ci95"], atol=1e-9)

    ex = build_example()
    for b_arg, s in ((paths[1], ref), ("random", ref_random)):
        out = subprocess.run([ex, paths[0], b_arg, str(P), "--seed", str(seed), "--json"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        same(json.loads(out.stdout.strip().splitlines()[-1]), s)
    out = subprocess.run([ex, paths[0], "random", "64"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "score" in out.stdout, out.stderr
    fp = build_facade_probe()
    out = subprocess.run([fp, paths[0], paths[1], str(P), str(seed)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    same(json.loads(out.stdout.strip().splitlines()[-1]), ref)
    ar.close(), da.close(), db.close()


def test_invalid_arguments():
    with pytest.raises(xq.XqError):
        Arena(0)
    ar = Arena(4)
    small = xq.DQN((1260, 32, 64), seed=1)                     # fewer than 90 outputs
    with pytest.raises(xq.XqError):
        ar.run(small, None)
    with pytest.raises(xq.XqError):
        ar.reset(201)
    ar.close(), small.close()
