"""GPU tests of versus training (DESIGN.md §4 "Versus training") — `pytest -m gpu`.

(1) 24 collects + updates against random play, search-1, search-2 (eps 0.1) and a borrowed network, replayed on the CPU restatement
    (tests/versus_ref.py) with the device's own Q values: boards, meta, every ring slot, episode records and outcome counters bit for bit,
    parameters within the trainer tolerance of the fp64 oracle TD update;
(2) set_opponent(X) then set_opponent(None) leaves self-play bit for bit;
(3) the borrowed opponent network is left as it was, and its stream does not change the learner's bits;
(4) overlap_collect equals its sequential definition;
(5) the bench composition at full size against search-1 keeps every ring slot invariant;
(6) invalid arguments, and the facade.
"""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import versus_ref as vr
import xqoracle as xo
from ring_window_ref import overlap_window
from test_dqn_gpu import oracle_td_update, REF_NET, CFG2_NET, PTOL

pytestmark = pytest.mark.gpu

VALUE = np.array([0, 1000, 20, 20, 40, 90, 45, 10, 1000, 20, 20, 40, 90, 45, 10], dtype=np.int64)


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def config(xq, n, cap, minibatch, seed, first, sizes=REF_NET, lr=0.01, eps=0.1, **kw):
    return xq.TrainerConfig(n_games=n, layer_sizes=sizes, learning_rate=lr, gamma=0.99, epsilon=eps, replay_capacity=cap,
                            minibatch=minibatch, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=seed,
                            first_game_id=first, **kw)


def opponent(xq, kind, sizes=REF_NET, stream=None):
    """-> (the Trainer.set_opponent argument, the restatement's Opponent without Q, the borrowed net or None)"""
    if kind == "random":
        return "random", vr.Opponent(vr.RANDOM), None
    if kind.startswith("search"):
        d = int(kind[-1])
        return xq.Search(d, 0.1), vr.Opponent(vr.SEARCH, eps=0.1, depth=d), None
    net = xq.DQN(sizes, 0.01, 0.99, seed=3, stream=stream)
    net.set_params(*xo.init_weights(sizes, 9))
    return (net, 0.1), vr.Opponent(vr.NET, eps=0.1), net


def q_rows(xq, env, d):
    """The device's Q rows (first 96 outputs) of a list of oracle boards, through d's forward on a scratch env."""
    def f(boards):
        env.set_state(np.stack([b.squares() for b in boards]))
        return d.q_boards(env, 96).cpu().numpy()
    return f


def material(boards, side):
    """evaluateBoard's material term for `side` (0 Red, 1 Black), per board: own pieces minus the other side's."""
    v = VALUE[boards.astype(np.int64)]
    red = (boards >= 1) & (boards <= 7)
    blk = boards >= 8
    m = (v * red).sum(1) - (v * blk).sum(1)
    return np.where(side == 0, m, -m)


@pytest.mark.parametrize("kind", ["random", "search1", "search2", "net"])
def test_versus_collects_replay_on_the_restatement(xq, kind):
    n, cap, mb, iters, seed, first, lr = 64, 512, 48, 24, 0x7E57, 5, 0.01
    t = xq.Trainer(config(xq, n, cap, mb, seed, first, lr=lr))
    t.dqn.set_params(*xo.init_weights(REF_NET, 21))
    arg, opp, net = opponent(xq, kind)
    t.set_opponent(arg)
    scratch = xq.VecEnv(n, seed=seed, first_game_id=first)
    learner = xq.DQN(REF_NET, lr, 0.99, seed=1)
    if net is not None:
        opp.q = q_rows(xq, scratch, net)
    # the games start late (moveCount 150..199): the 200-move cap ends some of them within the run, whatever the players do
    mc0 = [150 + (g * 7) % 50 for g in range(n)]
    t.env.set_state(np.tile(xq.START_BOARD, (n, 1)), np.array([[m, 0, 0, 0] for m in mc0]))
    games = [vr.Game(first + g, board=xo.board_from(xq.START_BOARD, mc0[g], 0)) for g in range(n)]
    results, episodes = [], []
    rseed = seed + 0x1234567 + first
    key = (rseed & 0xFFFFFFFF, rseed >> 32)
    for it in range(iters):
        w, b = t.dqn.get_params()
        learner.set_params(w, b)
        c = vr.Collect(seed, 0.1, opp)
        want = c.run(games, q_rows(xq, scratch, learner))
        results += c.results
        episodes += c.episodes
        t.collect()
        boards, meta = t.env.get_state()
        for g, game in enumerate(games):
            assert np.array_equal(boards[g], game.b.squares()), (it, g)
            assert list(meta[g]) == [game.b.moveCount, game.b.currentPlayer, game.b.redScore, game.b.blackScore], (it, g)
            s, a, r, dn, s2 = t.replay.get((it * n + g) % cap)
            ws, wa, wr, wd, ws2 = want[g]
            assert np.array_equal(s, ws) and np.array_equal(s2, ws2) and (a, r, dn) == (wa, float(wr), wd), (it, g)
        t.learn_grads()
        t.learn_apply(1)
        if it < 2 or it == iters - 1:          # the update against the fp64 oracle, on the minibatch re-derived from the ring's stream
            size = min(cap, (it + 1) * n)
            slots = [xo.philox((i, 0, it, 1), key)[0] % size for i in range(mb)]
            tr = [t.replay.get(s) for s in slots]
            keep = [x for x in tr if x[1] >= 0]          # an empty slot contributes no gradient
            S, A, R, D, S2 = (np.array([x[k] for x in keep]) for k in range(5))
            ww, wb, _, _ = oracle_td_update(REF_NET, w, b, w, b, S, A.astype(np.int64), R, D, S2, 0.99, lr, 1.0 / mb, 0)
            gw, gb = t.dqn.get_params()
            assert np.abs(gw - ww).max() < PTOL and np.abs(gb - wb).max() < PTOL, it
    got = t.versus_results()
    res = np.array([r for _, r in results])
    assert (got["wins"], got["draws"], got["losses"], got["games"]) == \
        (int((res == 1).sum()), int((res == 0).sum()), int((res == -1).sum()), len(res))
    rec, _ = t.env.drain_episodes()
    have = sorted((int(e["game_id"]), int(e["episode"]), int(e["red_score"]), int(e["black_score"]), int(e["move_count"]),
                   int(e["winner"]), int(e["reserved"])) for e in rec)
    assert have == sorted(episodes)
    assert t.counters()["env_steps"] == n * iters
    assert len(res) > 0 and (res == 0).sum() > 0
    t.close(); scratch.close(); learner.close()
    if net is not None:
        net.close()


def test_self_play_is_untouched_by_an_opponent_set_and_cleared(xq):
    n, cap, mb, iters, seed, first = 64, 256, 48, 7, 4242, 100
    out = []
    for with_opp in (False, True):
        t = xq.Trainer(config(xq, n, cap, mb, seed, first, sizes=CFG2_NET, eps=0.2))
        if with_opp:
            t.set_opponent(xq.Search(2, 0.3))
            t.set_opponent(None)
        t.random_plies(5)
        t.step(iters)
        w, b = t.dqn.get_params()
        boards, meta = t.env.get_state()
        out.append((w, b, boards, meta, t.env.counters(), t.counters(), t.replay.get(17)))
        t.close()
    (w0, b0, B0, M0, E0, C0, R0), (w1, b1, B1, M1, E1, C1, R1) = out
    assert np.array_equal(w0, w1) and np.array_equal(b0, b1) and np.array_equal(B0, B1) and np.array_equal(M0, M1)
    assert E0 == E1 and C0 == C1
    assert all(np.array_equal(x, y) for x, y in zip(R0, R1))


def test_the_borrowed_opponent_is_left_as_it_was(xq):
    import torch
    n, cap, mb, iters, seed, first = 256, 2048, 128, 50, 99, 3
    probe = xq.VecEnv(96, seed=5)
    for _ in range(7):
        probe.selfplay_step(None, 1.0)
    runs = []
    for shared in (False, True):
        s = torch.cuda.Stream() if shared else None
        sp = C.c_void_p(s.cuda_stream) if shared else None
        t = xq.Trainer(config(xq, n, cap, mb, seed, first, sizes=CFG2_NET), stream=sp)
        t.dqn.set_params(*xo.init_weights(CFG2_NET, 4))
        arg, _, net = opponent(xq, "net", sizes=CFG2_NET, stream=sp)
        twin = xq.DQN(CFG2_NET, 0.01, 0.99, seed=3)
        twin.set_params(*xo.init_weights(CFG2_NET, 9))
        q0 = net.select_q(probe).cpu().numpy()           # the select chain keeps state: both nets run it on the same boards
        twin.select_q(probe)
        net.kernel_stats(2)                              # statistics on and cleared
        w0, b0 = net.get_params()
        t.set_opponent(arg)
        t.step(iters)
        assert t.versus_results()["games"] > 0
        assert net.kernel_stats(0) == []                 # the trainer's forwards are not the handle's work
        w1, b1 = net.get_params()
        assert np.array_equal(w0, w1) and np.array_equal(b0, b1)
        # the select chain of the lent net continues exactly as the twin's that was never lent
        probe2 = xq.VecEnv(96, seed=6)
        qa, qb = net.select_q(probe2).cpu().numpy(), twin.select_q(probe2).cpu().numpy()
        assert np.array_equal(qa, qb) and q0.shape == (96, 96)
        runs.append(t.dqn.get_params())
        t.close(); net.close(); twin.close(); probe2.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    probe.close()


@pytest.mark.parametrize("n,cap,mb,plies,iters,kind", [(1024, 1 << 14, 1024, 1, 8, "search1"), (256, 4096, 512, 4, 5, "net")])
def test_overlapped_versus_trainer_equals_its_sequential_definition(xq, n, cap, mb, plies, iters, kind):
    """As test_overlapped_trainer_equals_its_sequential_definition: the collects are those of a second, sequential trainer that is
    only ever asked to collect, with theta_t copied into it."""
    import torch
    seed, first, lr = 99, 7, 0.01
    kw = dict(collects_per_update=plies)
    t = xq.Trainer(config(xq, n, cap, mb, seed, first, sizes=CFG2_NET, lr=lr, overlap_collect=1, **kw))
    w0, b0 = t.dqn.get_params()
    arg, _, net = opponent(xq, kind, sizes=CFG2_NET)
    t.set_opponent(arg)
    t.step(iters)
    tw, tb = t.dqn.get_params()
    tboards, tmeta = t.env.get_state()
    tres = t.versus_results()

    c = xq.Trainer(config(xq, n, cap, mb, seed, first, sizes=CFG2_NET, lr=lr, **kw))
    c.set_opponent(arg)
    d = xq.DQN(CFG2_NET, lr, 0.99, seed=1)
    d.set_params(w0, b0)
    rp = c.replay
    m = n * plies

    def collect():
        c.dqn.set_params(*d.get_params())
        for _ in range(plies):
            c.collect()
        c.synchronize()
        torch.cuda.synchronize()

    for it in range(iters):
        size, _, total = rp.stats()
        start, count = overlap_window(size, total, cap, m)
        if count <= 0:
            collect()
            rp.sample(mb)
            d.td_grads_replay(rp, mb, td_net=0, mode=0)
        else:
            rp.sample_window(mb, start, count)
            d.td_grads_replay(rp, mb, td_net=0, mode=0)
            collect()
        d.apply_grads(lr, 1.0 / mb)
    w, b = d.get_params()
    boards, meta = c.env.get_state()
    assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
    assert np.array_equal(w, tw) and np.array_equal(b, tb)
    keys = ("wins", "draws", "losses", "games")
    assert [c.versus_results()[k] for k in keys] == [tres[k] for k in keys]
    assert np.abs(w - w0).max() > 0
    t.close(); c.close(); d.close()
    if net is not None:
        net.close()


def test_full_size_against_search1_keeps_every_slot_invariant(xq):
    from cn_chess_ai_amd import _capi
    n, cap, seed, iters = 8192, 1 << 20, 0x5EED, 200
    t = xq.Trainer(config(xq, n, cap, n, seed, 0, sizes=CFG2_NET, lr=0.001, overlap_collect=1, collects_per_update=1))
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.dqn.set_fused_apply(True)
    t.random_plies(300)
    ep0 = t.counters()["episodes"]
    t.set_opponent(xq.Search(1))
    t.step(iters)
    c = t.counters()
    assert c["env_steps"] == n * iters and c["updates"] == iters
    res = t.versus_results()
    assert res["wins"] + res["draws"] + res["losses"] == res["games"] == c["episodes"] - ep0 > 0
    size, _, total = t.replay.stats()
    assert size == cap and total == n * iters
    # every slot of the ring: learner = (first_game_id + g) & 1 with g = slot % n (cap is a multiple of n)
    rng = np.random.default_rng(1)
    idx = np.sort(rng.choice(cap, 20000, replace=False))
    rows = [t.replay.get(int(i)) for i in idx]
    S, A, R, D, S2 = (np.array([r[k] for r in rows]) for k in range(5))
    side = (idx % n) & 1
    mat = material(S2, side)
    # reward = trunc(material - 0.1 moveCount) with 0 <= moveCount <= 200 (learner's view; the mover's view has the other sign)
    lo, hi = np.trunc(mat - 20.0), mat
    empty = A < 0
    ok = empty & (R == 0) & (D == 1) | ~empty & (R >= lo) & (R <= hi)
    assert ok.all(), np.nonzero(~ok)[0][:10]
    # on a sample: s has the learner to move (its `to` is a learner move of s) and s' follows from s by that move and one reply, or done
    rng = np.random.default_rng(2)
    for k in rng.choice(len(idx), 400, replace=False):
        if A[k] < 0:
            continue
        me = int(side[k])
        b = xo.board_from(S[k], 0, me)
        codes, _ = xo.all_valid_actions(b, me)
        mine = [int(x) for x in codes if int(x) % 90 == A[k]]
        assert mine, k
        if D[k]:
            continue
        reach = False
        for code in mine:
            b1 = xo.board_from(S[k], 0, me)
            f, to = divmod(code, 90)
            xo.lib().xqo_move_piece(C.byref(b1), f // 9, f % 9, to // 9, to % 9)
            for rc in xo.all_valid_actions(b1, 1 - me)[0]:
                b2 = xo.board_from(b1.squares(), 0, 1 - me)
                f2, t2 = divmod(int(rc), 90)
                xo.lib().xqo_move_piece(C.byref(b2), f2 // 9, f2 % 9, t2 // 9, t2 % 9)
                if np.array_equal(b2.squares(), S2[k]):
                    reach = True
                    break
            if reach:
                break
        assert reach, k
    t.close()


def test_invalid_arguments_and_the_facade(xq, tmp_path):
    from cn_chess_ai_amd import _capi
    t = xq.Trainer(config(xq, 64, 256, 32, 1, 0))
    h = t._h
    bad = [_capi.ArenaPlayer(7, None, 0, 0.0), _capi.ArenaPlayer(_capi.PLAYER_SEARCH, None, 0, 0.0),
           _capi.ArenaPlayer(_capi.PLAYER_SEARCH, None, 4, 0.0), _capi.ArenaPlayer(_capi.PLAYER_SEARCH, None, 1, -0.1),
           _capi.ArenaPlayer(_capi.PLAYER_SEARCH, None, 1, 1.5), _capi.ArenaPlayer(_capi.PLAYER_NET, None, 0, 0.0),
           _capi.ArenaPlayer(_capi.PLAYER_NET, t.dqn.handle, 0, 0.0)]
    small = xq.DQN([1260, 64, 80], 0.01, 0.99, seed=1)
    other = xq.DQN([630, 64, 8100], 0.01, 0.99, seed=1)
    bad += [_capi.ArenaPlayer(_capi.PLAYER_NET, small.handle, 0, 0.0), _capi.ArenaPlayer(_capi.PLAYER_NET, other.handle, 0, 0.0)]
    lib = _capi.load()
    for p in bad:
        assert lib.xq_trainer_set_opponent(h, C.byref(p)) == 1, (p.kind, p.depth, p.eps)     # XQ_ERR_INVALID_ARGUMENT
    with pytest.raises(TypeError):
        t.set_opponent(xq.Search)
    # between iterations only
    t.set_opponent(xq.Search(1))
    t.collect()
    t.learn_grads()
    with pytest.raises(xq.XqError):
        t.set_opponent(None)
    t.learn_apply(1)
    t.set_opponent(None)
    t.close(); small.close(); other.close()
    # the facade: the sequential loop refuses an opponent, the batched one trains against search-1
    from test_versus_cpu import build_versus_facade_probe
    exe = build_versus_facade_probe()
    out = subprocess.run([exe, "256", "300", "7", "1"], check=True, capture_output=True, text=True, timeout=600).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r["refused"] == 1
    assert r["wins"] + r["draws"] + r["losses"] == r["ended"] > 0 and r["env_steps"] > 0
