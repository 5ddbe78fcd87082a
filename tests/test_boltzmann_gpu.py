"""The Boltzmann pick of the env kernel and the settable epsilon, held to tests/boltzmann_ref.py — `pytest -m gpu`.

Every DECIDED draw of the reference (outside its band, boltzmann_ref's docstring) must be the kernel's move, and at most 2 % of the draws
of a case may be undecided.  The inputs of the crafted-board tests are tests/boltzmann_edge_cases.py's, on which
tests/test_boltzmann_ref_cpu.py holds the reference to an fp32 emulation of the device rule.  The slab forms, versus training and the
arena run on network rows: the reference then reads the fp32 row of xq_dqn_forward_boards_dev, whose bits the slab forms promise.
"""
import numpy as np
import pytest

import argmax_edge_cases as ac
import boltzmann_edge_cases as be
import boltzmann_ref as bz
import first_max as fm
from test_first_maximum_gpu import expected_moves, play, slab_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def eps_u32(eps):
    return int(min(max(float(eps), 0.0) * 4294967296.0, 4294967295.0))


# ---------------------------------------------------------------------------------------------------------------- crafted boards
def crafted_step(xq, T, eps=0.0, q_view=False, policy=True):
    inp = be.inputs()
    env = xq.VecEnv(be.N_GAMES, seed=be.SEED)
    try:
        env.set_state(inp["boards"], inp["meta"])
        if q_view:
            env.set_q_view(True)
        if policy:
            env.set_policy("boltzmann", T)
        res = env.selfplay_step(inp["q"], eps)
        counters = env.counters()
    finally:
        env.close()
    return res, counters


def check_against_reference(res, want, what):
    n_of = np.array([len(c) for c in be.inputs()["lists"]])
    assert np.array_equal(res["n_moves"], n_of), what
    live = n_of > 0
    assert (res["action"][~live] == -1).all() and (res["explored"][~live] == 0).all(), what
    share = float(want["undecided"][live].mean())
    decided = live & ~want["undecided"]
    bad = np.nonzero(decided & ((res["action"] != want["action"]) | (res["explored"] != want["explored"])))[0]
    other = int((live & want["undecided"] & (res["action"] != want["action"])).sum())
    print(f"BOLTZMANN {what}: {int(decided.sum())} decided draws, undecided {share:.5f} ({other} resolved the other way), "
          f"explored == 2 on {np.mean(res['explored'][live] == 2):.3f}")
    assert share <= bz.MAX_UNDECIDED, (what, share)
    assert len(bad) == 0, (what, len(bad), [(int(g), be.inputs()["pattern"][g], int(n_of[g]), int(res["action"][g]), int(want["action"][g]),
                                              int(res["explored"][g]), int(want["explored"][g])) for g in bad[:8]])


@pytest.mark.parametrize("T", be.TEMPS)
def test_crafted_boards_follow_the_reference(xq, T):
    res, counters = crafted_step(xq, T)
    check_against_reference(res, be.expected(T), f"crafted T {T}")
    assert counters["explored"] == 0                     # the counter keeps counting epsilon plies only


def test_composition_with_epsilon(xq):
    T, eps = 0.25, be.EPS_COMPOSED
    res, counters = crafted_step(xq, T, eps)
    never, _ = crafted_step(xq, T, eps, policy=False)    # a never-asked env on the same seed
    want = be.expected(T, eps=eps)
    check_against_reference(res, want, f"composed with eps {eps}")
    R = be.philox_words()
    n_of = np.array([len(c) for c in be.inputs()["lists"]])
    took = (R[:, 0] < eps_u32(eps)) & (n_of > 0)
    assert 0.25 * be.N_GAMES < took.sum() < 0.35 * be.N_GAMES
    assert np.array_equal(res["action"][took], never["action"][took]) and (res["explored"][took] == 1).all()
    assert (never["explored"][took] == 1).all() and (never["explored"][~took] == 0).all()
    for g in np.nonzero(took)[0]:
        assert int(res["action"][g]) == int(be.inputs()["lists"][g][int(R[g, 1]) % n_of[g]]), g
    assert counters["explored"] == int(took.sum())


def test_q_view_reads_the_swapped_square(xq):
    T = 1.0
    res, _ = crafted_step(xq, T, q_view=True)
    want, plain = be.expected(T, q_view=True), be.expected(T)
    black = be.inputs()["meta"][:, 1] == 1
    assert (want["action"][black] != plain["action"][black]).sum() > 100       # the swap decides the move in many Black games
    assert np.array_equal(want["action"][~black], plain["action"][~black])
    check_against_reference(res, want, "q-view")


# ---------------------------------------------------------------------------------------------------------------- never asked
def play_50_plies(xq, setup, eps):
    """50 plies of 256 games on random device rows with a ring -> everything the plies left behind, as bytes"""
    import torch
    from cn_chess_ai_amd.vecenv import STEP_DTYPE
    n, plies = 256, 50
    env = xq.VecEnv(n, seed=0x5EED + 3)
    ring = xq.ReplayBuffer(n * plies, seed=5)
    out = []
    try:
        setup(env)
        g = torch.Generator(device="cpu").manual_seed(11)
        rd = torch.zeros(n * STEP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        for ply in range(plies):
            qd = (torch.rand(n, 96, generator=g) * 2 - 1).cuda()
            torch.cuda.synchronize()
            env.selfplay_step_dev(qd.data_ptr(), 96, eps, results_dev=rd.data_ptr(), replay=ring)
            S, M = env.get_state()                       # (a blocking copy on the env's stream: the ply is over)
            torch.cuda.synchronize()
            out += [rd.cpu().numpy().tobytes(), S.tobytes(), M.tobytes()]
        out.append(repr(sorted(env.counters().items())).encode())
        for slot in range(n * plies):                    # the ring: every slot of every ply
            b, a, r, d, nb = ring.get(slot)
            out.append(b.tobytes() + nb.tobytes() + np.array([a, d], np.int32).tobytes() + np.float32(r).tobytes())
    finally:
        ring.close(); env.close()
    return out


def test_an_env_set_back_to_greedy_is_an_env_never_asked(xq):
    def there_and_back(env):
        env.set_policy("boltzmann", 0.5)
        env.set_policy("greedy", 0.5)
    fresh = play_50_plies(xq, lambda env: None, 0.1)
    assert play_50_plies(xq, there_and_back, 0.1) == fresh
    # ... and the comparison can fail: the policy left on moves the games
    assert play_50_plies(xq, lambda env: env.set_policy("boltzmann", 0.5), 0.1) != fresh


def test_at_epsilon_one_the_temperature_is_inert(xq):
    assert play_50_plies(xq, lambda env: env.set_policy("boltzmann", 0.5), 1.0) == play_50_plies(xq, lambda env: None, 1.0)


# ---------------------------------------------------------------------------------------------------------------- fed by the network
T_NET = 0.25


def reference_moves(q, lists, R, T):
    """the reference's (index, undecided) per game on network rows; -1 without a move"""
    idx, und = np.full(len(lists), -1), np.zeros(len(lists), bool)
    for g, codes in enumerate(lists):
        if len(codes):
            idx[g], _, und[g] = bz.step(q[g], codes, T, R[g])
    return idx, und


def run_collect(xq, net, pattern, overlap, versus=False):
    import torch
    sizes = [1260] + [int(s) for s in net.split("-")]
    n, seed = 2048, 0x5EED + 7
    w, b = slab_params(sizes, pattern)
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=sizes, learning_rate=0.01, gamma=0.99, epsilon=0.0, replay_capacity=4096, minibatch=n,
                           td_net=0, backprop_mode=1, target_sync_interval=0, seed=seed, first_game_id=0, overlap_collect=overlap)
    t = xq.Trainer(cfg)
    d = xq.DQN(sizes, 0.01, 0.99, seed=1)
    opp = xq.DQN([1260, 64, 90], 0.01, 0.99, seed=2) if versus else None
    twin = xq.VecEnv(n, seed=seed, first_game_id=0)
    try:
        t.dqn.set_params(w, b)
        t.dqn.updateTargetNetwork()
        d.set_params(w, b)
        t.set_policy("boltzmann", T_NET)
        assert t.env.policy() == ("boltzmann", T_NET)
        if versus:
            t.set_opponent((opp, 0.0))
        t.random_plies(25)
        assert t.env.counters()["plies"] == 25 * n                      # every slot's ply counter stands at 25
        S0, M0 = t.env.get_state()
        t.collect()
        torch.cuda.synchronize()
        S1, _ = t.env.get_state()
        ring = [t.replay.get(g) for g in range(n)]
        S = np.stack([r[0] for r in ring])                              # the boards the learner moved on
        M = M0.copy()
        learner = np.arange(n) & 1                                      # versus: the learner is Black in the odd games
        premoved = (M0[:, 1] != learner) if versus else np.zeros(n, bool)
        if versus:
            M[:, 1] = learner
            # phase 0: where the opponent was to move it played the first maximum of ITS rows — no draw
            qo, lo, po = expected_moves(xq, opp, twin, S0, M0, 90)
            for g in np.nonzero(premoved)[0]:
                if ring[g][1] >= 0 and po[g] >= 0:
                    assert np.array_equal(S[g], play(S0[g], lo[g][po[g]])[0]), (g, "pre-move")
        q, lists, _ = expected_moves(xq, d, twin, S if versus else S0, M)
        R = be.philox_words(n, seed, 0, 25 + premoved.astype(np.int64))
        idx, und = reference_moves(q, lists, R, T_NET)
        after = np.zeros((n, 90), np.uint8)
        checked = moved = 0
        for g in range(n):
            _, a, _, done, nb = ring[g]
            if versus and a < 0:                                        # the game ended on the opponent's pre-move
                continue
            if idx[g] < 0:
                assert a < 0, (net, pattern, g, a)
                continue
            if und[g]:
                continue
            code = lists[g][idx[g]]
            after[g], taken = play(S[g], code)
            assert a == int(code) % 90, (net, pattern, overlap, g, a, int(code) % 90)
            if not versus:
                assert np.array_equal(S1[g], xq.START_BOARD if taken in (1, 8) else after[g]), (net, pattern, overlap, g)
                if not done:
                    assert np.array_equal(nb, after[g]), (net, pattern, overlap, g)
            moved += idx[g] != fm.pick(q[g], lists[g])
            checked += 1
        if versus:
            # phase 2: the opponent's reply to the learner's draw is the first maximum of its rows again
            Ma = M.copy()
            Ma[:, 1] ^= 1
            ok = np.array([ring[g][1] >= 0 and idx[g] >= 0 and not und[g] and not ring[g][3] for g in range(n)])
            qo, lo, po = expected_moves(xq, opp, twin, after, Ma, 90)
            for g in np.nonzero(ok)[0]:
                assert np.array_equal(ring[g][4], play(after[g], lo[g][po[g]])[0]), (g, "reply")
            assert ok.sum() > 0.8 * n
        share = float(und.mean())
        print(f"BOLTZMANN collect {net} {pattern} overlap {overlap} versus {int(versus)}: {checked} decided draws, undecided {share:.5f}, "
              f"left the first maximum {moved / max(checked, 1):.3f}")
        assert share <= bz.MAX_UNDECIDED, share
        assert checked >= (0.88 * n if versus else 0.97 * n), checked
        if pattern != "inf_weight":
            assert moved > 0.1 * checked, moved                         # the draw is no first maximum in disguise
    finally:
        t.close(); twin.close(); d.close()
        if opp is not None:
            opp.close()


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("pattern", ["dup_sets", "sat50", "inf_weight"])
@pytest.mark.parametrize("net", list(ac.SLAB_NETS))
def test_collect_draws_from_the_forward_row(xq, net, pattern, overlap):
    run_collect(xq, net, pattern, overlap)


def test_versus_learner_draws_and_a_net_opponent_stays_greedy(xq):
    run_collect(xq, "128-640-8100", "dup_sets", 1, versus=True)


# ---------------------------------------------------------------------------------------------------------------- arena
def test_arena_ply_q_dev_draws_for_a_alone(xq):
    import torch
    from cn_chess_ai_amd.arena import Arena
    P, opening, seed, T = 512, 2, 0x5EED + 9, 1.0
    ar, plain = Arena(P, seed=seed, opening_plies=opening), Arena(P, seed=seed, opening_plies=opening)
    twin = xq.VecEnv(2 * P)
    try:
        ar.set_temperature(T, 0.0)
        assert ar.temperature() == (T, 0.0)
        rng = np.random.default_rng(3)
        live = np.ones(2 * P, bool)
        drawn = greedy = 0
        for ply in range(opening + 4):
            q = np.zeros((2 * P, 96), np.float32)
            q[:, :90] = rng.uniform(-1, 1, (2 * P, 90))
            qd = torch.from_numpy(q).cuda()
            torch.cuda.synchronize()
            S, M = ar.env.get_state()
            ar.ply_q_dev(qd)
            res = ar.last_step()
            if ply < opening:                                           # the opening is nobody's policy
                plain.ply_q_dev(qd)
                assert res.tobytes() == plain.last_step().tobytes(), ply
                continue
            twin.set_state(S, M)
            codes, counts = twin.legal_moves()
            R = be.philox_words(2 * P, seed, 0, ply)
            a_moves = (ply % 2 == 0) == (np.arange(2 * P) < P)
            for g in np.nonzero(live)[0]:
                lst = codes[g, :counts[g]]
                if len(lst) == 0:
                    continue
                idx, expl, und = bz.step(q[g, :90], lst, T if a_moves[g] else None, R[g])
                if und:
                    continue
                assert int(res[g]["action"]) == int(lst[idx]) and int(res[g]["explored"]) == expl, (ply, g, bool(a_moves[g]))
                drawn += a_moves[g] and expl == 2
                greedy += (not a_moves[g]) and expl == 0
            live &= res["terminated"] == 0
        assert drawn > P and greedy > 1.5 * P, (drawn, greedy)
        ar.reset(opening)
        assert ar.temperature() == (T, 0.0)                             # survives a reset
    finally:
        ar.close(); plain.close(); twin.close()


def test_a_temperature_tells_the_games_of_one_opening_apart(xq):
    from cn_chess_ai_amd.arena import Arena
    sizes = [1260, 64, 90]
    d = xq.DQN(sizes, 0.01, 0.99, seed=4)
    P = 64
    ar = Arena(P, seed=0x5EED + 10, opening_plies=0)
    try:
        def sequences():
            ar.reset(0)
            moves = []
            for _ in range(10):
                ar.run(d, d, 0.0, 0.0, max_plies=1)
                moves.append(ar.last_step()["action"].copy())
            m = np.stack(moves, axis=1)
            return len({tuple(r) for r in m[:P]}), len({tuple(r) for r in m[P:]})
        assert sequences() == (1, 1)                                    # two deterministic players: one game per seat
        ar.set_temperature(1.0, 1.0)
        a, b = sequences()
        print(f"BOLTZMANN arena at T = 1: {a} and {b} distinct 10-ply games among {P} per seat")
        assert a > 1 and b > 1
        ar.set_temperature(0.0, 0.0)
        assert sequences() == (1, 1)
    finally:
        ar.close(); d.close()


# ---------------------------------------------------------------------------------------------------------------- setters
def test_setters_refuse_what_they_must_and_change_nothing_then(xq):
    from cn_chess_ai_amd.arena import Arena
    env = xq.VecEnv(4)
    ar = Arena(2)
    cfg = xq.TrainerConfig(n_games=64, layer_sizes=[1260, 64, 90], epsilon=0.1, replay_capacity=256, minibatch=64, target_sync_interval=0)
    t = xq.Trainer(cfg)
    try:
        assert env.policy() == ("greedy", 1.0)
        env.set_policy("boltzmann", 0.5)
        for bad in (0.0, -1.0, 1e-4, 9.99e-4, 1001.0, 1e4, float("nan"), float("inf"), -float("inf"), 1e300):
            for kind in ("boltzmann", "greedy"):
                with pytest.raises(xq.XqError):
                    env.set_policy(kind, bad)
            with pytest.raises(xq.XqError):
                t.set_policy("boltzmann", bad)
        with pytest.raises(xq.XqError):
            env.set_policy(7, 1.0)
        with pytest.raises(ValueError):
            env.set_policy("softmax", 1.0)
        assert env.policy() == ("boltzmann", 0.5)
        env.set_policy("greedy", 2.0)                                   # checked, kept, not used
        assert env.policy() == ("greedy", 2.0)
        for ok in (1e-3, 1e3):
            env.set_policy("boltzmann", ok)
            assert env.policy() == ("boltzmann", ok)
        t.set_policy("boltzmann", 0.75)
        assert t.env.policy() == ("boltzmann", 0.75)
        assert t.epsilon() == 0.1
        for bad in (-0.1, 1.0001, float("nan"), float("inf")):
            with pytest.raises((xq.XqError, ValueError)):
                t.set_epsilon(bad)
            with pytest.raises(xq.XqError):
                xq._capi.call("xq_trainer_set_epsilon", t._h, bad)
        assert t.epsilon() == 0.1
        for ok in (0.0, 1.0, 0.3):
            t.set_epsilon(ok)
            assert t.epsilon() == ok
        assert ar.temperature() == (0.0, 0.0)
        ar.set_temperature(0.5, 0.0)
        for bad in (-1.0, 1e-4, 1e4, float("nan"), float("inf")):
            with pytest.raises(xq.XqError):
                ar.set_temperature(bad, 0.0)
            with pytest.raises(xq.XqError):
                ar.set_temperature(0.0, bad)
        assert ar.temperature() == (0.5, 0.0)
    finally:
        t.close(); ar.close(); env.close()


@pytest.mark.parametrize("overlap", [0, 1])
def test_set_epsilon_takes_effect_at_the_next_collect(xq, overlap):
    n = 2048
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=[1260, 64, 8100], epsilon=0.0, replay_capacity=8 * n, minibatch=256, target_sync_interval=0,
                           seed=0x5EED + 12, overlap_collect=overlap)
    t = xq.Trainer(cfg)
    try:
        t.set_policy("boltzmann", 1.0)                                  # a Boltzmann draw is no epsilon ply
        seen = []
        for eps in (0.0, 0.5, 0.1, 1.0, 0.0):
            t.set_epsilon(eps)
            before = t.env.counters()["explored"]
            t.collect()
            t.set_epsilon(eps)                                          # legal with the collect still in flight and a learn_grads to come
            t.learn_grads()
            t.learn_apply()
            seen.append((t.env.counters()["explored"] - before) / float(n))
        print(f"BOLTZMANN set_epsilon overlap {overlap}: explored share per setting {seen}")
        assert seen[0] == 0.0 and seen[4] == 0.0 and seen[3] > 0.999
        assert abs(seen[1] - 0.5) < 0.05 and abs(seen[2] - 0.1) < 0.03        # 2048 plies: > 4 sigma
    finally:
        t.close()
