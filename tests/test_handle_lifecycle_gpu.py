"""Creation and teardown of the handles' streams and events (`pytest -m gpu`): xq::Stream, xq::Event and xq::LazyMark of
csrc/xq_internal.h seen from the C ABI.  tests/test_stream_order_gpu.py destroys env, ring and Q-net on lent streams once per case, after
long sequences; here every handle kind goes away right after its first operation, over and over, with the lent stream destroyed the
moment the handle is gone — and what is built next, very likely at the recycled addresses, must neither find a stale entry of a dead
stream in a ring's bookkeeping nor a dead event.  Then the lazily created events of versus training, and trainers whose
construction fails half way.  Every error below is an API error (XQ_ERR_INVALID_ARGUMENT); nothing here provokes a GPU fault.
"""
import ctypes as C

import numpy as np
import pytest

from cn_chess_ai_amd import _capi

pytestmark = pytest.mark.gpu

GAMES, RING, NET, PAIRS, BATCH = 64, 256, (1260, 32, 96), 32, 48
MODE = _capi.BACKPROP_TEXTBOOK          # (a net this narrow is outside what the reference's backprop can address: XQ_ERR_UNDEFINED_UPSTREAM)
ROUNDS = 8


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def dsync():
    import torch
    torch.cuda.synchronize()


def new_stream(xq):
    h = C.c_void_p()
    xq._capi.call("xq_stream_create", 0, 0, C.byref(h))
    assert h.value
    return h


def trainer_config(xq, **kw):
    args = dict(n_games=GAMES, layer_sizes=NET, learning_rate=0.01, epsilon=0.1, replay_capacity=RING, minibatch=BATCH, td_net=0, backprop_mode=MODE,
                target_sync_interval=0, seed=7, overlap_collect=1)
    args.update(kw)
    return xq.TrainerConfig(**args)


# one handle of each kind on `stream` (None: a stream of its own), one small operation, gone again
def churn_env(xq, stream):
    e = xq.VecEnv(GAMES, seed=3, stream=stream)
    e.selfplay_step_dev(0, 96, 0.1)
    e.close()


def churn_ring(xq, stream):
    r = xq.ReplayBuffer(RING, seed=11, stream=stream)
    b = np.tile(np.asarray(xq.START_BOARD, np.uint8).reshape(1, 90), (4, 1))
    r.push(b, np.arange(4), np.zeros(4), np.zeros(4), b)
    r.sample(8, host=False)
    r.close()


def churn_dqn(xq, stream):
    d = xq.DQN(NET, 0.01, 0.99, seed=1, stream=stream)
    d.updateTargetNetwork()
    d.close()


def churn_arena(xq, stream):
    a = xq.Arena(PAIRS, seed=5, stream=stream)
    a.run(None, None, max_plies=2)
    a.close()


def churn_trainer(xq, stream):
    t = xq.Trainer(trainer_config(xq), stream=stream)
    t.step(1)
    t.close()


CHURN = [churn_env, churn_ring, churn_dqn, churn_arena, churn_trainer]


def ply_then_td_step(xq, streams):
    """One self-play ply into a ring, one TD step on it; env, ring and Q-net on streams[0..2] -> (Q(s,a), y) of the minibatch"""
    env = xq.VecEnv(GAMES, seed=3, stream=streams[0])
    rp = xq.ReplayBuffer(RING, seed=11, stream=streams[1])
    d = xq.DQN(NET, 0.01, 0.99, seed=1, stream=streams[2])
    env.selfplay_step_dev(0, 96, 0.1, replay=rp)
    rp.sample_window(GAMES, 0, GAMES, host=False)
    d.td_grads_replay(rp, GAMES, td_net=0, mode=MODE)
    q, y = d.last_td_values(GAMES)
    d.close(); rp.close(); env.close()
    return q, y


def test_lent_streams_destroyed_right_behind_their_handles(xq):
    for churn in CHURN:
        for _ in range(ROUNDS):
            s = new_stream(xq)
            churn(xq, s)
            xq._capi.call("xq_stream_destroy", s)
        for _ in range(ROUNDS):
            churn(xq, None)
    two = [new_stream(xq), new_stream(xq), None]          # env and ring on fresh streams, the Q-net on its own
    q2, y2 = ply_then_td_step(xq, two)
    for s in two[:2]:
        xq._capi.call("xq_stream_destroy", s)
    one = new_stream(xq)
    q1, y1 = ply_then_td_step(xq, [one, one, one])
    xq._capi.call("xq_stream_destroy", one)
    assert np.isfinite(q1).all() and np.isfinite(y1).all() and np.abs(q1).max() > 0
    assert q2.tobytes() == q1.tobytes() and y2.tobytes() == y1.tobytes()


def test_trainer_with_an_opponent_then_without(xq):
    """xq_trainer_set_opponent creates the versus events and buffers on first use; they go with the handle"""
    t = xq.Trainer(trainer_config(xq))
    t.set_opponent(xq.Search(1))
    t.step(1)
    c = t.counters()
    assert (c["env_steps"], c["updates"]) == (GAMES, 1)
    t.close()
    t = xq.Trainer(trainer_config(xq))
    t.step(1)
    c = t.counters()
    assert (c["env_steps"], c["updates"]) == (GAMES, 1)
    w, b = t.dqn.get_params()
    assert np.isfinite(w).all() and np.isfinite(b).all()
    t.close()


@pytest.mark.parametrize("broken", [dict(prioritized=1, replay_capacity=0, overlap_collect=0),
                                    dict(precision=_capi.PRECISION_BF16, layer_sizes=(1260, 33, 96))],
                         ids=["prioritized_without_a_ring", "bf16_with_an_odd_hidden_width"])
def test_trainer_whose_construction_fails_half_way(xq, broken):
    """Both configurations pass xq_trainer_create's own checks and fail inside the construction, after env, Q-net and ring exist"""
    for stream in (None, new_stream(xq)):
        with pytest.raises(xq.XqError) as err:
            xq.Trainer(trainer_config(xq, **broken), stream=stream)
        assert err.value.code == 1                       # XQ_ERR_INVALID_ARGUMENT
        t = xq.Trainer(trainer_config(xq), stream=stream)
        t.step(1)
        c = t.counters()
        assert (c["env_steps"], c["updates"]) == (GAMES, 1)
        t.close()
        if stream is not None:
            xq._capi.call("xq_stream_destroy", stream)
    dsync()
