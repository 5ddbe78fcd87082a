"""The mover view through the trainer (xq_trainer_set_view, DESIGN.md §4 "Mover view") — `pytest -m gpu`: 20 overlapped iterations of
self-play (legal bootstrap, zero-sum) and 20 of versus "random", each held bit for bit to the sequential definition
collect -> tests/view_ref.py -> the existing host step.  16 games, minibatch 16, a ring of 8 collects."""
import numpy as np
import pytest

import view_ref as vr
from test_legal_ring_gpu import ring_rows
from ring_window_ref import overlap_window

pytestmark = pytest.mark.gpu

SIZES = [1260, 64, 64, 8100]
N, MB, CAP, ITERS, SEED, FIRST, LR, EPS = 16, 16, 128, 20, 99, 7, 0.01, 0.2


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def config(xq, overlap, td_net):
    return xq.TrainerConfig(n_games=N, layer_sizes=SIZES, learning_rate=LR, gamma=0.99, epsilon=EPS, replay_capacity=CAP, minibatch=MB,
                            td_net=td_net, backprop_mode=0, target_sync_interval=3, mean_gradient=1, seed=SEED, first_game_id=FIRST,
                            collects_per_update=1, overlap_collect=overlap)


def host_step(d, rp, slots, td_net, legal):
    """the step of the definition: the sampled rows as the ring holds them (absolute), through view_ref, into the existing host step"""
    S, A, R, D, S2 = ring_rows(rp, slots)
    v = vr.apply(S, A, S2, rp.mover()[slots], rp.next_player()[slots])
    d.td_update(v["boards"], v["next_boards"], v["action"], R, D, td_net=td_net, learning_rate=LR, grad_scale=1.0 / MB,
                next_player=v["next_player"] if legal else None)
    return v


def run_definition(rp, collect, step):
    """xq_trainer_step's overlapped order: the minibatch is drawn from the ring without the slots this iteration's collect writes, the
    collect runs on theta_t, then the update"""
    for it in range(ITERS):
        size, _, total = rp.stats()
        start, count = overlap_window(size, total, CAP, N)
        if count <= 0:
            collect()
            slots = rp.sample(MB)
        else:
            slots = rp.sample_window(MB, start, count)
            collect()
        step(slots, it)


def test_overlapped_selfplay_trainer_under_the_view_equals_its_sequential_definition(xq):
    import torch
    t = xq.Trainer(config(xq, 1, 1))
    env = xq.VecEnv(N, seed=SEED, first_game_id=FIRST)
    probe = xq.VecEnv(N, seed=1)
    d = xq.DQN(SIZES, LR, 0.99, seed=1)
    rp = xq.ReplayBuffer(CAP, seed=SEED + 0x1234567 + FIRST)
    try:
        t.set_td_bootstrap("legal")
        t.set_zero_sum(True)
        t.set_view("mover")
        w0, b0 = t.dqn.get_params()
        t.step(ITERS)
        tw, tb = t.dqn.get_params()
        tboards, tmeta = t.env.get_state()
        tf = t.dqn.last_view(MB)
        d.set_params(w0, b0); d.updateTargetNetwork()
        d.set_td_bootstrap("legal"); d.set_zero_sum(True)
        rp.track_mover(); rp.track_next_player()
        env.set_q_view(True)
        sides = []

        def collect():
            boards, meta = env.get_state()
            sides.append(meta[:, 1].copy())
            probe.set_state(vr.view(boards, meta[:, 1]))             # the host-built view, read as it stands
            q = d.q_boards(probe, 96)
            env.selfplay_step_dev(q.data_ptr(), 96, EPS, replay=rp)
            torch.cuda.synchronize()

        last = {}

        def step(slots, it):
            last["v"] = host_step(d, rp, slots, 1, True)
            if (it + 1) % 3 == 0:
                d.updateTargetNetwork()

        run_definition(rp, collect, step)
        w, b = d.get_params()
        boards, meta = env.get_state()
        assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
        assert np.array_equal(w, tw) and np.array_equal(b, tb) and np.abs(w - w0).max() > 0
        assert np.array_equal(rp.mover(0, CAP), t.replay.mover(0, CAP)) and np.array_equal(rp.next_player(0, CAP), t.replay.next_player(0, CAP))
        assert set(np.unique(np.concatenate(sides))) == {0, 1}       # both colours moved
        for k in ("flag_s", "flag_next", "boards", "next_boards", "action"):
            assert np.array_equal(tf[k], last["v"][k]), k
        assert np.array_equal(tf["flag_next"], 1 - tf["flag_s"])
    finally:
        t.close(); env.close(); probe.close(); d.close(); rp.close()


def test_overlapped_versus_trainer_under_the_view_equals_its_sequential_definition(xq):
    """the collects are those of a second, sequential trainer under the view that is only ever asked to collect, with theta_t copied into
    it (tests/test_versus_gpu.py's arrangement); the step is the definition's"""
    import torch
    t = xq.Trainer(config(xq, 1, 0))
    c = xq.Trainer(config(xq, 0, 0))
    d = xq.DQN(SIZES, LR, 0.99, seed=1)
    try:
        for x in (t, c):
            x.set_opponent("random")
            x.set_view("mover")
        w0, b0 = t.dqn.get_params()
        t.step(ITERS)
        tw, tb = t.dqn.get_params()
        tboards, tmeta = t.env.get_state()
        tres = t.versus_results()
        d.set_params(w0, b0)
        rp = c.replay

        def collect():
            c.dqn.set_params(*d.get_params())
            c.collect()
            c.synchronize()
            torch.cuda.synchronize()

        run_definition(rp, collect, lambda slots, it: host_step(d, rp, slots, 0, False))
        w, b = d.get_params()
        boards, meta = c.env.get_state()
        assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
        assert np.array_equal(w, tw) and np.array_equal(b, tb) and np.abs(w - w0).max() > 0
        keys = ("wins", "draws", "losses", "games")
        assert [c.versus_results()[k] for k in keys] == [tres[k] for k in keys]
        colour = (FIRST + np.arange(N)) & 1
        assert np.array_equal(rp.mover(0, CAP).reshape(-1, N), np.tile(colour, (CAP // N, 1)))
        assert np.array_equal(rp.mover(0, CAP), t.replay.mover(0, CAP)) and np.array_equal(rp.next_player(0, CAP), t.replay.next_player(0, CAP))
    finally:
        t.close(); c.close(); d.close()
