"""Workspace growth gives the same bits (`pytest -m gpu`): one DQN handle run at a small batch, then larger ones, then small again
computes, at every stage, exactly what a fresh handle that only ever saw that stage's size computes from the same parameters.

Every workspace of the handle is sized by the largest batch it has seen, so the grown handle works in buffers that are larger than
the stage needs and still hold what the larger stages left in them; the fresh handle's are exact and new.  The stages are chosen so
that each family of buffers grows at least once on the way up:
  256  : the step's own buffers (ensure_capacity), the matrix-pipe layer-0 gradient's planes (n >= 256), the select chain's kept sums;
  1024 : the smallest batch whose max pass runs on 128-row tiles (64 x 8 tiles >= 512), i.e. the first that screens: the screening
         buffers and their candidate counters are allocated here ...
  2048 : ... and grow here (the counters' totals are carried over on the host), with the k-slabs of the select head (n >= 2048).
"""
import numpy as np
import pytest

import xqoracle as xo
from test_dqn_gpu import CFG2_NET

pytestmark = pytest.mark.gpu

STAGES = (256, 1024, 2048, 1024, 256)
NAMES = ("q_boards", "select_q", "select_q (derived)", "qsa", "y", "weights", "biases")


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def _handle(xq, precision, qmax_mode):
    d = xq.DQN(CFG2_NET, 0.001, 0.99, seed=1)
    d.set_precision(precision)
    d.set_qmax_mode(qmax_mode)
    d.set_l0_derive(True)          # fp32 net: the select chain keeps its layer-0 sums from the second call of an update period on
    return d


def _stage(xq, d, n, params, td_net):
    """One stage at batch n from fixed parameters: n seeded games, six random plies into a ring of n slots, then the board forward,
    the select path twice (the second call derives from the sums the first kept) and one TD step over the ring."""
    import torch
    (w, b), (wt, bt) = params
    d.set_params(w, b)
    d.set_params(wt, bt, net=1)
    env = xq.VecEnv(n, seed=1000 + n)
    rp = xq.ReplayBuffer(n, seed=7)
    for _ in range(6):
        env.selfplay_step_dev(replay=rp)
    torch.cuda.synchronize()
    assert rp.stats()[0] == n
    out = [d.q_boards(env, 96).cpu().numpy(), d.select_q(env).cpu().numpy(), d.select_q(env).cpu().numpy()]
    d.td_grads_replay(rp, 0, td_net=td_net, mode=0)
    d.apply_grads(0.05, 1.0 / n)
    out += list(d.last_td_values(n))
    out += list(d.get_params())
    env.close(); rp.close()
    return out


@pytest.mark.parametrize("precision,td_net,qmax_mode", [(0, 1, 1), (2, 2, 0)], ids=["fp32-screened", "bf16full-double"])
def test_workspace_growth_gives_the_same_bits(xq, precision, td_net, qmax_mode):
    """fp32 net, target-net rule, screened max pass (the headline's shape of step) and the bf16-full net under Double DQN (bf16 copies of
    every activation buffer, the third forward chain and the arg-max partials grow too).  Q values of both forward routes, Q(s, a) and y
    of the TD step and the parameters after it are compared byte for byte (NaN-safe) at every stage."""
    w, b = xo.init_weights(CFG2_NET, 21)
    b = np.random.default_rng(22).uniform(-0.05, 0.05, size=len(b))
    wt, bt = xo.init_weights(CFG2_NET, 23)
    params = ((w, b), (wt, bt))
    grown = _handle(xq, precision, qmax_mode)
    screened = [0, 0, 0, 0]
    for stage, n in enumerate(STAGES):
        got = _stage(xq, grown, n, params, td_net)
        fresh = _handle(xq, precision, qmax_mode)
        want = _stage(xq, fresh, n, params, td_net)
        screened = [a + c for a, c in zip(screened, fresh.qmax_stats())]
        fresh.close()
        assert np.abs(want[5] - w).max() > 0                       # the step really moved the weights
        for name, g, f in zip(NAMES, got, want):
            assert g.shape == f.shape and g.tobytes() == f.tobytes(), (stage, n, name, int((g != f).sum()))
    # the screen ran where it should, and the candidate counters of the arrays the grown handle replaced were carried over
    assert list(grown.qmax_stats()) == screened
    assert screened[0] == (3 if qmax_mode else 0) and screened[1] == (1024 + 2048 + 1024 if qmax_mode else 0)
    grown.close()
