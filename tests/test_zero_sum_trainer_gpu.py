"""The zero-sum target through the trainer (xq_trainer_set_zero_sum, DESIGN.md §4 "Zero-sum target") — `pytest -m gpu`: it and
set_opponent refuse each other, Trainer.set_zero_sum is DQN.set_zero_sum on the trainer's net (the same parameters after 5 iterations,
overlap_collect 0 and 1, n_step 1 and 3, default rule and legal bootstrap with the delta reward), and each such run differs from the run
without it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
GAMES, MINIBATCH, RING, ITERS = 64, 64, 4096, 5


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def trainer(xq, overlap=0, prioritized=0):
    cfg = xq.TrainerConfig(n_games=GAMES, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=0.97, epsilon=0.3, replay_capacity=RING,
                           minibatch=MINIBATCH, td_net=1, target_sync_interval=3, seed=21, overlap_collect=overlap,
                           prioritized=prioritized, per_alpha=0.6, per_beta=0.4, per_eps=1e-3)
    return xq.Trainer(cfg)


def test_zero_sum_and_an_opponent_refuse_each_other(xq):
    t = trainer(xq, overlap=1)
    try:
        assert t.dqn.zero_sum() is False
        with pytest.raises(ValueError):
            t.set_zero_sum(1)
        t.set_opponent("random")
        with pytest.raises(xq.XqError) as e:
            t.set_zero_sum(True)
        assert e.value.code == 1 and "xq_trainer_set_opponent" in str(e.value)
        assert t.dqn.zero_sum() is False
        t.set_zero_sum(False)                                  # off is always allowed
        t.step(1)                                              # versus training goes on
        t.set_opponent(None)
        t.set_zero_sum(True)
        assert t.dqn.zero_sum() is True
        for opp in ("random", xq.Search(1, 0.1)):
            with pytest.raises(xq.XqError) as e:
                t.set_opponent(opp)
            assert e.value.code == 1 and "xq_trainer_set_zero_sum" in str(e.value)
        t.set_opponent(None)                                   # self-play again is no conflict
        t.step(1)
        # between iterations only
        t.learn_grads()
        with pytest.raises(xq.XqError) as e:
            t.set_zero_sum(False)
        assert e.value.code == 2 and t.dqn.zero_sum() is True
        t.collect(); t.learn_apply(1)
        t.set_zero_sum(False)
        assert t.dqn.zero_sum() is False
        t.set_opponent("random")
        t.step(1)
    finally:
        t.close()


def run(xq, how, overlap, n_step, legal_delta, prioritized=0):
    t = trainer(xq, overlap, prioritized)
    try:
        if legal_delta:
            t.set_td_bootstrap("legal")
            t.set_reward("delta", 1e-3, 0.0, 1.0)
        if n_step > 1:
            t.set_n_step(n_step)
        if how == "trainer":
            t.set_zero_sum(True)
        elif how == "net":
            t.dqn.set_zero_sum(True)
        assert t.dqn.zero_sum() is (how != "off")
        t.step(ITERS)
        w, b = t.dqn.get_params()
        q, y = t.dqn.last_td_values(MINIBATCH)
        assert t.counters()["updates"] == ITERS and np.isfinite(w).all() and np.isfinite(y).all()
        return w, b, q, y
    finally:
        t.close()


@pytest.mark.parametrize("legal_delta", [False, True], ids=["all_evaluate", "legal_delta"])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("overlap", [0, 1])
def test_trainer_setter_is_the_nets_setter_and_the_flag_is_live(xq, overlap, n_step, legal_delta):
    wa, ba, qa, ya = run(xq, "trainer", overlap, n_step, legal_delta)
    wb, bb, qb, yb = run(xq, "net", overlap, n_step, legal_delta)
    wc, bc, qc, yc = run(xq, "off", overlap, n_step, legal_delta)
    assert np.array_equal(wa, wb) and np.array_equal(ba, bb) and np.array_equal(qa, qb) and np.array_equal(ya, yb)
    assert np.abs(wa - wc).max() > 0 and not np.array_equal(ya, yc)


def test_prioritized_ring(xq):
    wa, ba, qa, ya = run(xq, "trainer", 1, 3, False, prioritized=1)
    wb, bb, qb, yb = run(xq, "net", 1, 3, False, prioritized=1)
    wc, _, _, yc = run(xq, "off", 1, 3, False, prioritized=1)
    assert np.array_equal(wa, wb) and np.array_equal(ba, bb) and np.array_equal(ya, yb)
    assert np.abs(wa - wc).max() > 0


def test_on_policy_ring(xq):
    outs = {}
    for how in ("trainer", "net", "off"):
        cfg = xq.TrainerConfig(n_games=GAMES, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=0.97, epsilon=0.3, replay_capacity=0,
                               minibatch=GAMES, td_net=1, target_sync_interval=3, seed=21)
        t = xq.Trainer(cfg)
        try:
            if how == "trainer":
                t.set_zero_sum(True)
            elif how == "net":
                t.dqn.set_zero_sum(True)
            t.step(ITERS)
            outs[how] = np.concatenate(t.dqn.get_params())
        finally:
            t.close()
    assert np.array_equal(outs["trainer"], outs["net"]) and np.abs(outs["trainer"] - outs["off"]).max() > 0
