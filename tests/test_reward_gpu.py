"""The reward rule (xq_env_set_reward, DESIGN.md §4 "Reward rule") on the device — `pytest -m gpu`.

(1) self-play: 32 games x 120 plies into a ring under delta(1/1000, 0.003, inf) — every slot's reward bit for bit the reference's, from
    the ring's own s / s' and from the oracle replay; again with bound 0.5 (clamps the general) and with a Q policy at epsilon 0.1;
(2) versus: 32 games x 80 collects against random play and search-1 against tests/reward_ref.py's Collect, every slot; a hand-built
    position that ends in the opponent's pre-move keeps reward 0;
(3) an env that was never asked, one asked for "evaluate" and one switched to delta and back write the same bits; a switch mid-run
    changes only the slots written afterwards; the step result keeps evaluateBoard;
(4) composition: n-step returns and the TD target read the delta column; the trainer matrix writes it;
(5) refusals, and the facade.

The parameters 1/1000 and 0.003 are the ones at which a fused multiply-add rounds delta = 10, 40 and 1000 differently
(tests/test_reward_ref_cpu.py), so a kernel that contracts the product fails (1) and (2)."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest

import nstep_ref as nr
import reward_ref as rr
import versus_ref as vr
import xqoracle as xo
from test_dqn_gpu import REF_NET, make_net

pytestmark = pytest.mark.gpu

SEED, FIRST, N, PLIES, COLLECTS = 0x5EED, 1000, 32, 120, 80
PARAMS = (1.0 / 1000, 0.003, np.inf)
SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.97


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def columns(rp, slots):
    rows = [rp.get(int(s)) for s in slots]
    S, A, R, D, S2 = (np.array([r[k] for r in rows]) for k in range(5))
    return S, A.astype(np.int32), R.astype(np.float32), D.astype(np.uint8), S2


@pytest.fixture(scope="module")
def oracle_random():
    """the reference run: uniform-random self-play on the CPU oracle, every ply's (s, to, captured value, mover, s', evaluate, done)"""
    sp = rr.SelfPlay(N, SEED, FIRST)
    plies = [sp.step() for _ in range(PLIES)]
    assert set(sp.victims) == {1, 2, 3, 4, 5, 6, 7}, sp.victims           # every victim type, generals included
    return plies


def play(xq, plies, reward=None, q=None, eps=1.0, results=False):
    """`plies` self-play plies of N games into a fresh ring (reward: the set_reward arguments, or a list of (ply, arguments) switches)
    -> env, ring[, the step results of every ply]"""
    import torch
    env = xq.VecEnv(N, seed=SEED, first_game_id=FIRST)
    rp = xq.ReplayBuffer(N * plies, seed=1)
    switches = reward if isinstance(reward, list) else ([(0, reward)] if reward is not None else [])
    qd = None
    if q is not None:
        qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).cuda()
    res = torch.zeros((plies, N, xq.vecenv.STEP_DTYPE.itemsize), dtype=torch.uint8, device="cuda") if results else None
    torch.cuda.synchronize()
    for t in range(plies):
        for at, args in switches:
            if at == t:
                env.set_reward(*args)
        env.selfplay_step_dev(qd[t].data_ptr() if qd is not None else 0, 96, eps, res[t].data_ptr() if results else None, rp)
    env.get_state(0, 1)                                                    # (synchronises the env's stream)
    if results:
        torch.cuda.synchronize()
        return env, rp, res.cpu().numpy().view(xq.vecenv.STEP_DTYPE).reshape(plies, N)
    return env, rp


def assert_selfplay_ring(rp, plies, params):
    S, A, R, D, S2 = columns(rp, range(N * len(plies)))
    for t, rows in enumerate(plies):
        for g, (s, to, value, mover, s2, _, done) in enumerate(rows):
            k = t * N + g
            assert np.array_equal(S[k], s) and np.array_equal(S2[k], s2) and (A[k], D[k]) == (to, done), (t, g)
            want = rr.formula(value, *params)
            assert bits(R[k]) == bits(want), (t, g, value, R[k], want)                     # the oracle replay's capture
            assert bits(R[k]) == bits(rr.ring_reward(S[k], A[k], S2[k], params)), (t, g)   # the ring's own two boards


# ---- 1. self-play --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", [np.inf, 0.5])
def test_selfplay_ring_rewards_equal_the_reference(xq, oracle_random, bound):
    params = (PARAMS[0], PARAMS[1], bound)
    env, rp = play(xq, PLIES, ("delta",) + params)
    try:
        assert env.reward == ("delta",) + params
        assert_selfplay_ring(rp, oracle_random, params)
        _, _, R, _, _ = columns(rp, range(N * PLIES))
        if np.isfinite(bound):
            assert (R == np.float32(bound)).sum() >= 1 and (np.abs(R) <= np.float32(bound)).all()    # the general is clamped
        else:
            assert R.max() == rr.formula(1000, *params) > 0.99
    finally:
        env.close(); rp.close()


def test_selfplay_ring_rewards_under_a_q_policy(xq):
    q = np.random.default_rng(7).standard_normal((PLIES, N, 96)).astype(np.float32)
    sp = rr.SelfPlay(N, SEED, FIRST)
    plies = [sp.step(q[t][:, :90], 0.1) for t in range(PLIES)]
    assert len(sp.victims) >= 5
    env, rp = play(xq, PLIES, ("delta",) + PARAMS, q=q, eps=0.1)
    try:
        assert_selfplay_ring(rp, plies, PARAMS)
        assert 0 < env.counters()["explored"] < N * PLIES // 4
    finally:
        env.close(); rp.close()


# ---- 2. versus -----------------------------------------------------------------------------------------------------------------------
def versus_config(xq, n, cap, **kw):
    return xq.TrainerConfig(n_games=n, layer_sizes=REF_NET, learning_rate=0.01, gamma=0.99, epsilon=1.0, replay_capacity=cap, minibatch=n,
                            td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=SEED, first_game_id=FIRST, **kw)


def assert_versus_slots(got, want, params, where):
    S, A, R, D, S2 = got
    for g, (s, to, r, done, s2) in enumerate(want):
        assert np.array_equal(S[g], s) and np.array_equal(S2[g], s2) and (A[g], D[g]) == (to, done), (where, g)
        assert bits(R[g]) == bits(r), (where, g, R[g], r)
        if not (to < 0 and isinstance(r, int)):                       # (not the empty slot of a pre-move that ended the game)
            assert bits(R[g]) == bits(rr.ring_reward(S[g], A[g], S2[g], params, (FIRST + g) & 1)), (where, g)


@pytest.mark.parametrize("kind", ["random", "search1"])
def test_versus_ring_rewards_equal_the_reference(xq, kind):
    opp = vr.Opponent(vr.RANDOM) if kind == "random" else vr.Opponent(vr.SEARCH, eps=0.0, depth=1)
    slots, deltas, results = rr.versus_run(N, COLLECTS, SEED, FIRST, opp, PARAMS)
    ds = [d for _, d, _, _, _ in deltas]
    if kind == "random":                                                  # the conditions on the reference run
        assert 1000 in ds and -1000 in ds
        assert any(took > 0 and lost > 0 for _, _, took, lost, _ in deltas)
    else:
        assert -1000 in ds                                                # the search takes the general it is offered
    t = xq.Trainer(versus_config(xq, N, N * COLLECTS))
    try:
        t.set_reward("delta", *PARAMS)
        t.set_opponent("random" if kind == "random" else xq.Search(1))
        for _ in range(COLLECTS):
            t.collect()
        t.synchronize()
        S, A, R, D, S2 = columns(t.replay, range(N * COLLECTS))
        for c, want in enumerate(slots):
            sl = slice(c * N, (c + 1) * N)
            assert_versus_slots((S[sl], A[sl], R[sl], D[sl], S2[sl]), want, PARAMS, c)
        res = t.versus_results()
        rs = [r for _, r in results]
        assert (res["wins"], res["draws"], res["losses"]) == (rs.count(1), rs.count(0), rs.count(-1))
    finally:
        t.close()


def test_versus_games_that_end_without_a_learner_move(xq):
    """tests/test_versus_cpu.py's position — one side has no piece left and is to move.  Even ids (the learner is Red): the opponent's
    pre-move ends the game, the empty slot keeps reward 0.  Odd ids (the learner is Black): the learner has no move, delta = 0."""
    board = np.zeros(90, np.uint8)
    board[0 * 9 + 4], board[4 * 9 + 4] = 1, 5                             # Red general and chariot, Black to move
    params = (1e-3, 0.25, 1.0)
    games = [vr.Game(FIRST + g, board=xo.board_from(board, 20, 1)) for g in range(N)]
    c = rr.DeltaCollect(SEED, 1.0, vr.Opponent(vr.RANDOM), params)
    want = c.run(games, None)
    t = xq.Trainer(versus_config(xq, N, N * 4))
    try:
        t.set_reward("delta", *params)
        t.set_opponent("random")
        t.env.set_state(np.tile(board, (N, 1)), np.array([[20, 1, 0, 0]] * N))
        t.collect()
        t.synchronize()
        got = columns(t.replay, range(N))
        assert_versus_slots(got, want, params, "hand-built")
        A, R = got[1], got[2]
        assert (A == -1).all()
        assert (R[0::2] == 0).all() and (bits(R[1::2]) == bits(np.float32(-0.25))).all()
    finally:
        t.close()


# ---- 3. never asked, switched ---------------------------------------------------------------------------------------------------------
def test_evaluate_is_an_env_that_was_never_asked(xq):
    plies, out = 40, []
    # never asked; asked for the default; delta and back (with other parameters, which the default rule does not use) before the first ply
    for reward in (None, ("evaluate",), [(0, ("delta",) + PARAMS), (0, ("evaluate", 0.5, 0.125, 3.0))]):
        env, rp = play(xq, plies, reward)
        if reward is None:
            assert env.reward == ("evaluate", 1e-3, 0.0, 1.0)             # the defaults
        out.append(columns(rp, range(N * plies)) + (env.get_state(), env.counters()))
        env.close(); rp.close()
    base = out[0]
    for other in out[1:]:
        for a, b in zip(base[:5], other[:5]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert np.array_equal(base[5][0], other[5][0]) and np.array_equal(base[5][1], other[5][1]) and base[6] == other[6]
    assert np.abs(base[2]).max() > 100                                    # evaluateBoard: the material balance itself


def test_delta_then_evaluate_writes_evaluate(xq, oracle_random):
    plies = 12
    env, rp = play(xq, plies, [(0, ("delta",) + PARAMS), (0, ("evaluate",))])
    try:
        assert env.reward[0] == "evaluate"
        _, _, R, _, _ = columns(rp, range(N * plies))
        want = np.array([float(row[5]) for rows in oracle_random[:plies] for row in rows], dtype=np.float32)
        assert np.array_equal(bits(R), bits(want))
    finally:
        env.close(); rp.close()


def test_switch_mid_run_changes_only_later_slots(xq, oracle_random):
    plies, at = 40, 17
    env, rp, res = play(xq, plies, [(at, ("delta",) + PARAMS)], results=True)
    try:
        _, _, R, _, _ = columns(rp, range(N * plies))
        rows = [row for rows in oracle_random[:plies] for row in rows]
        evaluate = np.array([float(r[5]) for r in rows], dtype=np.float32)
        delta = np.array([rr.formula(r[2], *PARAMS) for r in rows], dtype=np.float32)
        assert np.array_equal(bits(R[:at * N]), bits(evaluate[:at * N])) and np.array_equal(bits(R[at * N:]), bits(delta[at * N:]))
        assert not np.array_equal(bits(evaluate[at * N:]), bits(delta[at * N:]))
        # the step result is evaluateBoard under either rule
        assert np.array_equal(res["reward"].reshape(-1), np.array([r[5] for r in rows]))
    finally:
        env.close(); rp.close()


# ---- 4. composition -------------------------------------------------------------------------------------------------------------------
def test_n_step_and_td_target_read_the_delta_column(xq):
    plies = PLIES                                                     # (the run in which generals fall: rows that end an episode)
    env, rp = play(xq, plies, ("delta", 1e-3, 0.0, 1.0))
    d, _, _ = make_net(xq, SMALL_NET, seed=3, gamma=GAMMA)
    try:
        size = N * plies
        _, A, R, D, _ = columns(rp, range(size))
        assert ((D == 1) & (A >= 0)).sum() >= 1 and (R > 0).sum() > 10 and R.max() == 1.0
        d.td_grads_replay(rp, 0)                                      # the identity batch
        _, y = d.last_td_values(size)
        ended = (D == 1) & (A >= 0)
        assert np.array_equal(bits(y[ended]), bits(R[ended]))         # y = r exactly where the transition ends the episode
        assert (np.abs(y[A >= 0]) <= 1.0 + GAMMA).all()
        d.apply_grads(0.0, 1.0)
        rp.set_n_step(3, N)
        d.td_grads_replay(rp, 0)
        got = d.last_n_step(size)
        ref = nr.assemble(A, R, D, size, np.arange(size, dtype=np.int32), 3, N, GAMMA, *nr.readable(size, size, 0))
        assert np.array_equal(bits(got["reward"]), bits(ref["reward"]))
        for k in ("done", "steps", "first_slot", "last_slot", "action"):
            assert np.array_equal(got[k], ref[k]), k
        d.apply_grads(0.0, 1.0)
    finally:
        env.close(); rp.close(); d.close()


@pytest.mark.parametrize("versus", [False, True])
@pytest.mark.parametrize("ring,overlap", [("uniform", 0), ("uniform", 1), ("prioritized", 0), ("prioritized", 1), ("on_policy", 0)])
def test_trainer_matrix_writes_the_delta_reward(xq, ring, overlap, versus):
    iters, spread = 8, 60
    cap = 0 if ring == "on_policy" else N * iters
    cfg = xq.TrainerConfig(n_games=N, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.3, replay_capacity=cap,
                           minibatch=N, td_net=1, target_sync_interval=3, seed=SEED, first_game_id=FIRST, overlap_collect=overlap,
                           prioritized=1 if ring == "prioritized" else 0)
    t = xq.Trainer(cfg)
    try:
        t.random_plies(spread)                                        # the games are spread over all phases: captures from the first ply on
        if versus:
            t.set_opponent("random")
        t.set_reward("delta", *PARAMS)
        assert t.env.reward == ("delta",) + PARAMS
        moved, seen = 0, 0
        for it in range(iters):
            before = t.replay.stats()[2]
            if overlap:
                t.learn_grads(); t.collect(); t.learn_apply(1)
            else:
                t.collect(); t.learn_grads(); t.learn_apply(1)
            t.synchronize()
            assert t.replay.stats()[2] == before + N
            S, A, R, D, S2 = columns(t.replay, range(N) if cap == 0 else range(it * N, (it + 1) * N))
            for g in range(N):
                side = (FIRST + g) & 1 if versus else None
                want = rr.ring_reward(S[g], A[g], S2[g], PARAMS, side)
                if versus and A[g] < 0 and R[g] == 0:
                    continue                                          # the empty slot of a pre-move that ended the game
                assert bits(R[g]) == bits(want), (it, g, R[g], want)
                seen += 1
                moved += want != rr.formula(0, *PARAMS)
        assert seen > N * iters * 3 // 4 and moved >= 3
        assert t.counters()["updates"] == iters
    finally:
        t.close()


# ---- 5. refusals, facade ----------------------------------------------------------------------------------------------------------------
def test_refusals(xq):
    inf, nan = np.inf, np.nan
    env = xq.VecEnv(N, seed=1)
    try:
        env.set_reward("delta", 0.25, 0.5, inf)
        bad = [(7, 1e-3, 0.0, 1.0), (-1, 1e-3, 0.0, 1.0), (1, 0.0, 0.0, 1.0), (1, -1e-3, 0.0, 1.0), (1, inf, 0.0, 1.0), (1, nan, 0.0, 1.0),
               (1, 1e-3, -0.1, 1.0), (1, 1e-3, inf, 1.0), (1, 1e-3, nan, 1.0), (1, 1e-3, 0.0, 0.0), (1, 1e-3, 0.0, -1.0), (1, 1e-3, 0.0, nan),
               (0, nan, 0.0, 1.0), (0, 1e-3, 0.0, -2.0)]
        for args in bad:
            assert not rr.args_ok(*args)
            with pytest.raises(xq.XqError) as e:
                env.set_reward(*args)
            assert e.value.code == 1, args
            assert env.reward == ("delta", 0.25, 0.5, inf)            # a refused call changes nothing
        with pytest.raises(ValueError):
            env.set_reward("material")
    finally:
        env.close()
    t = xq.Trainer(xq.TrainerConfig(n_games=N, layer_sizes=SMALL_NET, replay_capacity=N * 4, minibatch=N, seed=3))
    try:
        with pytest.raises(xq.XqError) as e:
            t.set_reward("delta", scale=-1.0)
        assert e.value.code == 1
        t.collect()
        t.learn_grads()
        with pytest.raises(xq.XqError) as e:                          # between iterations only
            t.set_reward("delta")
        assert e.value.code == 2 and t.env.reward[0] == "evaluate"
        t.learn_apply(1)
        t.set_reward("delta")
        assert t.env.reward == ("delta", 1e-3, 0.0, 1.0)
    finally:
        t.close()


def test_train_selfplay_reward_argument(xq, tmp_path):
    """the sequential loop refuses reward=delta (and trains nothing); the batched loop takes it"""
    from test_reward_ref_cpu import build_train_selfplay
    exe = build_train_selfplay()
    model = str(tmp_path / "model.bin")
    r = subprocess.run([exe, "2", model, "1", "reward=delta", "--save-every", "0"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Reward::delta needs the batched loop" in r.stderr, (r.returncode, r.stderr)
    r = subprocess.run([exe, "40", model, "64", "reward=delta:0.002:0.25:0.75", "--replay", "1024", "--minibatch", "64", "--save-every", "0",
                        "--seed", "7", "--json"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["updates"] > 0 and out["episodes_finished"] >= 40


def test_facade_carries_the_reward_onto_the_trainers_env(xq):
    from test_reward_ref_cpu import build_reward_facade_probe
    exe = build_reward_facade_probe()
    out = subprocess.run([exe, "64", "40", "7"], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r["env_before"] == [0, 1e-3, 0.0, 1.0] and r["env_after"] == [1, 0.002, 0.25, 1] and r["env_kept"] == 1
    assert r["env_refused"] == r["ai_refused"] == r["n_bad"] == 10
    assert (r["ai_before"], r["ai_after"]) == (0, 1)
    assert (r["train_refused"], r["episode_refused"], r["step_refused"], r["selfplay_refused"]) == (1, 1, 1, 1)
    assert r["plain"] == [0, 1e-3, 0.0, 1.0] and r["asked"] == [1, 0.002, 0.25, 0.75]
    assert r["plain_updates"] > 0 and r["asked_updates"] > 0
