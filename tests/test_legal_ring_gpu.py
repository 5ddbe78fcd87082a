"""The legal-move TD bootstrap from a replay ring and through the trainer (DESIGN.md §4 "Legal-move bootstrap") — `pytest -m gpu`.

4. The ring's side column: 1 - mover of every self-play transition, slot for slot, terminal plies included (the oracle's selfplay_step
   beside the device); the learner's colour in versus training; the refusals of a ring that holds transitions / of a plain push.
5. Composition: the step on a batch staged from a self-play ring (n-step, mirror, both; uniform and prioritized draws) equals the
   host-sided step on the same staged rows bit for bit, the side taken from the column at last_slot / slot.
6. Trainer: overlapped collect equals its sequential definition bit for bit under `legal`; `legal` after the first collect is refused.
"""
import numpy as np
import pytest

import xqoracle as xo
from test_dqn_gpu import CFG2_NET
from test_legal_gpu import GAMMA, SMALL_NET, bits, legal_net
from ring_window_ref import overlap_window

pytestmark = pytest.mark.gpu

PER = (0.6, 0.4, 1e-3)


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


# ---- 4. the column -----------------------------------------------------------------------------------------------------------------------
def test_selfplay_ring_records_one_minus_mover_slot_for_slot(xq):
    import torch
    n, plies, seed, eps = 96, 40, 21, 0.3
    env = xq.VecEnv(n, seed=seed)
    rp = xq.ReplayBuffer(n * plies, seed=4)
    try:
        rp.track_next_player()
        rp.track_next_player()                                               # a second call is a no-op
        # a third of the games start near the 200-ply cap: terminal plies and resets inside the run
        boards0, meta0 = env.get_state()
        meta0[: n // 3, 0] = 200 - 1 - np.arange(n // 3) % 7
        meta0[: n // 3, 1] = meta0[: n // 3, 0] & 1
        env.set_state(boards0, meta0)
        boards = [xo.board_from(boards0[g], *meta0[g]) for g in range(n)]
        rng = np.random.default_rng(5)
        want = np.zeros((plies, n), np.uint8)
        ended = 0
        for it in range(plies):
            q = rng.uniform(-1, 1, (n, 96)).astype(np.float32)
            for g in range(n):
                want[it, g] = 1 - boards[g].currentPlayer
                ended += xo.selfplay_step(boards[g], q[g, :90], seed, g, it, xo.eps_to_u32(eps)).done
            tq = torch.from_numpy(q).cuda()
            env.selfplay_step_dev(tq.data_ptr(), 96, eps, replay=rp)
            torch.cuda.synchronize()
        got, _ = env.get_state()
        assert all(np.array_equal(got[g], boards[g].squares()) for g in range(n))   # the oracle followed the device's games
        assert ended >= n // 3
        col = rp.next_player(0, n * plies).reshape(plies, n)
        assert np.array_equal(col, want) and set(np.unique(col)) == {0, 1}
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(boards0[:1], [3], [0.0], [0], boards0[:1])
        assert e.value.code == 1 and "push_host_sided" in str(e.value)
        rp.push(boards0[:2], [3, 4], [0.0, 0.5], [0, 1], boards0[:2], next_player=[1, 0])
        assert rp.next_player(0, 2).tolist() == [1, 0]
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(boards0[:1], [3], [0.0], [0], boards0[:1], next_player=[2])
        assert e.value.code == 1
    finally:
        env.close(); rp.close()


def test_tracking_needs_an_empty_ring_and_an_untracked_ring_has_no_column(xq):
    rp = xq.ReplayBuffer(8, seed=1)
    d = legal_net(xq, SMALL_NET)
    try:
        b = np.zeros((1, 90), np.uint8); b[0, 4], b[0, 85] = 1, 8
        with pytest.raises(xq._capi.XqError) as e:
            rp.next_player(0, 1)
        assert e.value.code == 2
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(b, [3], [0.0], [0], b, next_player=[0])
        assert e.value.code == 1 and "track_next_player" in str(e.value)
        rp.push(b, [3], [0.0], [0], b)
        with pytest.raises(xq._capi.XqError) as e:
            rp.track_next_player()
        assert e.value.code == 2 and "already holds" in str(e.value)
        with pytest.raises(xq._capi.XqError) as e:                              # legal from a ring without the column
            d.td_grads_replay(rp, 0)
        assert e.value.code == 1 and "track" in str(e.value)
    finally:
        rp.close(); d.close()


def test_versus_ring_records_the_learners_colour(xq):
    n, first = 64, 3
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.2, replay_capacity=n * 8,
                           minibatch=n, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=9,
                           first_game_id=first, collects_per_update=1, overlap_collect=0)
    t = xq.Trainer(cfg)
    try:
        t.set_opponent("random")
        t.set_td_bootstrap("legal")
        assert t.dqn.td_bootstrap() == "legal"
        t.step(5)
        col = t.replay.next_player(0, n * 5).reshape(5, n)
        assert np.array_equal(col, np.tile((first + np.arange(n)) & 1, (5, 1)))
        w, b = t.dqn.get_params()
        assert np.isfinite(w).all() and np.isfinite(b).all()
        L = t.dqn.last_legal(n, z96=False)
        assert (L["n_moves"] > 0).sum() > n // 2
    finally:
        t.close()


# ---- 5. composition ----------------------------------------------------------------------------------------------------------------------
def selfplay_ring(xq, n=64, plies=12, per=False):
    env = xq.VecEnv(n, seed=31)
    rp = xq.ReplayBuffer(n * plies, seed=5)
    rp.track_next_player()
    if per:
        rp.enable_per(*PER)
    for _ in range(25):
        env.selfplay_step(None)
    for _ in range(plies):
        env.selfplay_step_dev(0, 96, 1.0, replay=rp)
    env.get_state(0, 1)
    env.close()
    return rp


def ring_rows(rp, slots):
    rows = [rp.get(int(s)) for s in slots]
    return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.float32),
            np.array([r[3] for r in rows], np.uint8), np.stack([r[4] for r in rows]))


@pytest.mark.parametrize("n_step,mirror,per", [(3, 0.0, False), (1, 0.5, False), (3, 0.5, False), (1, 0.0, False), (1, 0.5, True),
                                               (1, 0.0, True)])
def test_staged_batch_step_equals_the_host_sided_step_on_the_staged_rows(xq, n_step, mirror, per):
    batch, lrate, n = 200, 0.05, 64
    rp = selfplay_ring(xq, n, per=per)
    g32 = np.float32(GAMMA)
    disc = np.float32(1.0)
    for _ in range(n_step):
        disc = np.float32(disc * g32)
    a = legal_net(xq, CFG2_NET)
    c = legal_net(xq, CFG2_NET)
    c2 = xq.DQN(CFG2_NET, 0.001, float(disc), seed=1)                            # the host step's discount: gamma^n as the device forms it
    try:
        c2.set_params(*a.get_params()); c2.set_params(*a.get_params(1), net=1); c2.set_td_bootstrap("legal")
        c.close(); c = c2
        if n_step > 1:
            rp.set_n_step(n_step, n)
        if mirror:
            rp.set_mirror(mirror)
        if per:
            rp.per_rebuild()
            slots, isw = rp.sample_prioritized(batch)
            before = rp.get_priorities(0, n * 12)
        else:
            slots = rp.sample(batch)
        a.td_grads_replay(rp, batch, td_net=2)
        a.apply_grads(lrate, 1.0 / batch)
        qa, ya = a.last_td_values(batch)
        La = a.last_legal(batch, z96=False)
        col = rp.next_player(0, n * 12)
        S, A, R, D, S2 = ring_rows(rp, slots)
        side_slot = slots
        if n_step > 1:
            ns = a.last_n_step(batch)
            assert np.array_equal(ns["first_slot"], slots)
            _, _, _, _, S2 = ring_rows(rp, np.maximum(ns["last_slot"], 0))
            A, R, D, side_slot = ns["action"], ns["reward"], ns["done"], np.maximum(ns["last_slot"], 0)
            assert (A >= 0).sum() > batch // 2
        if mirror:
            m = a.last_mirror(batch)
            assert np.array_equal(m["slot"], slots) and 0 < m["flags"].sum() < batch
            S, S2, A = m["boards"], m["next_boards"], m["action"]
        side = col[side_slot]
        assert set(np.unique(side)) == {0, 1}
        if per:
            # the host step has no importance weights: compare targets and the selection, and hold the written-back priorities to the
            # device's own Q(s,a) and legal y (batch_ref.priorities' formula)
            qc, yc = c.td_update(S, S2, A, R, D, td_net=2, learning_rate=0.0, grad_scale=1.0, next_player=side)
            assert np.array_equal(bits(qa), bits(qc)) and np.array_equal(bits(ya), bits(yc))
            after = rp.get_priorities(0, n * 12)
            live = A >= 0
            want = (np.abs(qa.astype(np.float64) - ya) + PER[2]) ** PER[0]
            last = {int(s): i for i, s in enumerate(slots) if live[i]}             # duplicates: any of them
            for s, i in last.items():
                dup = [j for j in range(batch) if slots[j] == s and live[j]]
                assert min(abs(after[s] / want[j] - 1) for j in dup) < 2e-5
            rest = np.setdiff1d(np.arange(n * 12), slots[live])
            assert np.array_equal(after[rest], before[rest])
        else:
            qc, yc = c.td_update(S, S2, A, R, D, td_net=2, learning_rate=lrate, grad_scale=1.0 / batch, next_player=side)
            assert np.array_equal(bits(qa), bits(qc)) and np.array_equal(bits(ya), bits(yc))
            for x, y in zip(a.get_params(), c.get_params()):
                assert np.array_equal(x, y)
        Lc = c.last_legal(batch, z96=False)
        for k in ("n_moves", "a_star"):
            assert np.array_equal(La[k], Lc[k]), k
        assert np.array_equal(bits(La["zmax"]), bits(Lc["zmax"]))
        assert (La["n_moves"] > 0).sum() > batch // 2
    finally:
        rp.close(); a.close(); c.close()


# ---- 6. trainer --------------------------------------------------------------------------------------------------------------------------
def test_overlapped_trainer_equals_its_sequential_definition_under_legal(xq):
    import torch
    n, cap, minibatch, iters, sizes, seed, first = 64, 256, 48, 20, CFG2_NET, 99, 7
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=sizes, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=cap,
                           minibatch=minibatch, td_net=1, backprop_mode=0, target_sync_interval=3, mean_gradient=1, seed=seed,
                           first_game_id=first, collects_per_update=1, overlap_collect=1)
    t = xq.Trainer(cfg)
    env = xq.VecEnv(n, seed=seed, first_game_id=first)
    d = xq.DQN(sizes, 0.01, 0.99, seed=1)
    rp = xq.ReplayBuffer(cap, seed=seed + 0x1234567 + first)
    try:
        t.set_td_bootstrap("legal")
        w0, b0 = t.dqn.get_params()
        t.step(iters)
        tw, tb = t.dqn.get_params()
        tboards, tmeta = t.env.get_state()
        assert t.dqn.last_legal(minibatch, z96=False)["n_moves"].max() > 0
        d.set_params(w0, b0); d.updateTargetNetwork()
        d.set_td_bootstrap("legal")
        rp.track_next_player()

        def collect():
            q = d.q_boards(env, 96)
            env.selfplay_step_dev(q.data_ptr(), 96, 0.2, replay=rp)
            torch.cuda.synchronize()

        for it in range(iters):
            size, _, total = rp.stats()
            start, count = overlap_window(size, total, cap, n)
            if count <= 0:
                collect()
                rp.sample(minibatch)
                d.td_grads_replay(rp, minibatch, td_net=1, mode=0)
            else:
                rp.sample_window(minibatch, start, count)
                d.td_grads_replay(rp, minibatch, td_net=1, mode=0)
                collect()
            d.apply_grads(0.01, 1.0 / minibatch)
            if (it + 1) % 3 == 0:
                d.updateTargetNetwork()
        w, b = d.get_params()
        boards, meta = env.get_state()
        assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
        assert np.array_equal(w, tw) and np.array_equal(b, tb) and np.abs(w - w0).max() > 0
        assert np.array_equal(rp.next_player(0, cap), t.replay.next_player(0, cap))
        t.set_td_bootstrap("all")
        assert t.dqn.td_bootstrap() == "all"
    finally:
        t.close(); env.close(); d.close(); rp.close()


def test_legal_after_the_first_collect_is_refused(xq):
    cfg = xq.TrainerConfig(n_games=32, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=128,
                           minibatch=32, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=3,
                           first_game_id=0, collects_per_update=1, overlap_collect=0)
    t = xq.Trainer(cfg)
    try:
        with pytest.raises(ValueError):
            t.set_td_bootstrap("some")
        t.collect()
        with pytest.raises(xq._capi.XqError) as e:
            t.set_td_bootstrap("legal")
        assert e.value.code == 2 and t.dqn.td_bootstrap() == "all"
        t.step(2)                                                                # the default rule goes on
    finally:
        t.close()
