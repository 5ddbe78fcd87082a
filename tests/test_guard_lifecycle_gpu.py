"""The screening guard of xq_dqn_set_qmax_mode over whole fallback cycles (`pytest -m gpu`): a handle is run for hundreds of TD steps and,
behind EVERY step, its screened-step count, fallback count and hold are those of tests/guard_model.py fed with the totals the device
reports (the model's own tests, and the negative control of the rule checked here: tests/test_guard_model_cpu.py).

CFG2_NET at n = 1024: the smallest batch that screens, exactly 32 refine blocks; n = 1100 needs 48, so the counter array is replaced.
The step size is 0: every step of a scenario computes the same thing, only the guard's state moves."""
import time

import numpy as np
import pytest

import xqoracle as xo
from guard_model import HOLD_STEPS, GuardModel
from test_dqn_gpu import CFG2_NET, _selfplay_transitions, make_net

pytestmark = pytest.mark.gpu

N, N_GROWN = 1024, 1100
TARGET = 1
NW_OUT = 8100 * 256


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def batches(xq):
    return {n: _selfplay_transitions(xq, n) for n in (N, N_GROWN)}


@pytest.fixture(scope="module")
def degenerate():
    """the all-rows-equal net of test_screened_qmax_degenerate_outputs: all 8100 outputs tie, every group is a candidate"""
    wt, bt = xo.init_weights(CFG2_NET, 79)
    wt = wt.copy()
    wt[-NW_OUT:] = np.tile(wt[-NW_OUT:-NW_OUT + 256], 8100)
    return wt, np.zeros(len(bt))


class Handle:
    """a Q-net whose TARGET net the TD rule reads (the online net is make_net's throughout), beside the model of its guard"""

    def __init__(self, xq, target):
        from cn_chess_ai_amd import _capi
        self.d, self.w, self.b = make_net(xq, CFG2_NET, seed=8)
        self.d.set_params(*target, net=TARGET)
        self.d.set_qmax_mode(_capi.QMAX_SCREENED)
        self.m = GuardModel()
        self.td_steps = 0
        self.t0 = time.perf_counter()

    def step(self, batch):
        """one TD step -> (screened, y); the guard's state behind it equals the model's"""
        _, y = self.d.td_update(*batch, td_net=TARGET, mode=0, learning_rate=0.0, grad_scale=1.0)
        self.td_steps += 1
        steps, samples, pairs, whole = self.d.qmax_stats()
        guard = self.d.qmax_guard()
        screened, fallbacks, hold = self.m.step(len(batch[0]), (pairs, whole))
        assert (steps, samples, guard) == (self.m.steps, self.m.samples, (fallbacks, hold)), \
            (self.td_steps, (steps, samples, guard), (self.m.steps, self.m.samples, fallbacks, hold), self.m.decisions)
        return screened, y

    def run(self, batch, steps):
        return [self.step(batch)[0] for _ in range(steps)]

    def close(self, name):
        print("%s: %d TD steps, %.2f s, decisions (S, S of the copy, fell back) %s"
              % (name, self.td_steps, time.perf_counter() - self.t0, self.m.decisions))
        self.d.close()


def run_to_first_fallback(h, batch):
    """64 screened steps of the degenerate net, then the first held one"""
    assert h.run(batch, 64) == [True] * 64
    assert h.step(batch)[0] is False and h.d.qmax_guard() == (1, HOLD_STEPS - 1)
    pairs, whole = h.d.qmax_stats()[2:]
    assert pairs >= 250 * 64 * N and whole >= 200 * 64 * N


def test_net_made_benign_during_the_hold_is_screened_for_good(xq, batches, degenerate):
    """Degenerate until the fallback, set_params(benign) in the middle of the hold: the hold runs out, the first screened step behind it
    has the bits of a fresh handle with the same two nets (parity slots, kept shadow rows), and the 160 steps behind that all screen —
    the window of the next decision holds nothing from before the hold."""
    from cn_chess_ai_amd import _capi
    batch = batches[N]
    h = Handle(xq, degenerate)
    run_to_first_fallback(h, batch)
    assert not any(h.run(batch, 255))
    h.d.set_params(h.w, h.b, net=TARGET)
    assert not any(h.run(batch, HOLD_STEPS - 256))
    assert h.d.qmax_guard() == (1, 0) and h.d.qmax_stats()[0] == 64
    f = xq.DQN(CFG2_NET, 0.001, 0.99, seed=8)
    for k in (0, 1):
        f.set_params(*h.d.get_params(k), net=k)
    f.set_qmax_mode(_capi.QMAX_SCREENED)
    before = h.d.qmax_stats()
    screened, y = h.step(batch)
    after = h.d.qmax_stats()
    _, y_f = f.td_update(*batch, td_net=TARGET, mode=0, learning_rate=0.0, grad_scale=1.0)
    assert screened and f.qmax_stats()[0] == 1
    assert np.array_equal(y.view(np.uint32), y_f.view(np.uint32))
    assert after[2] - before[2] == f.qmax_stats()[2] <= 24 * N        # the benign net is what the guard calls harmless
    assert h.run(batch, 160) == [True] * 160
    assert h.d.qmax_guard() == (1, 0) and h.d.qmax_stats()[0] == 64 + 161
    f.close(); h.close("degenerate, benign mid-hold")


def test_degenerate_throughout_is_held_again_after_64_screened_steps(xq, batches, degenerate):
    """TD steps 1..64 screen, 65..576 run the full product, 577..640 screen, 641 is held again; y of every tenth step, screened or
    not, stays within 2e-6 of one full-product y taken at the start."""
    from cn_chess_ai_amd import _capi
    batch = batches[N]
    h = Handle(xq, degenerate)
    h.d.set_qmax_mode(_capi.QMAX_FULL)
    _, y_full = h.d.td_update(*batch, td_net=TARGET, mode=0, learning_rate=0.0, grad_scale=1.0)
    y_full = y_full.copy()
    h.d.set_qmax_mode(_capi.QMAX_SCREENED)
    seen = []
    for t in range(1, 64 + HOLD_STEPS + 64 + 5 + 1):
        screened, y = h.step(batch)
        seen.append(screened)
        if t % 10 == 0:
            assert np.abs(y - y_full).max() < 2e-6, t
    assert seen == [True] * 64 + [False] * HOLD_STEPS + [True] * 64 + [False] * 5
    assert h.d.qmax_guard() == (2, HOLD_STEPS - 5)
    h.close("degenerate throughout")


def test_growth_while_a_copy_is_pending(xq, batches, degenerate):
    """40 screened steps at n = 1024 (the copy of step 32 is pending), then n = 1100: 48 refine blocks, the counter array is replaced,
    its totals carried, the pending copy dropped — and the net is caught on the next copy, at the model's step."""
    h = Handle(xq, degenerate)
    assert h.run(batches[N], 40) == [True] * 40 and h.m.pending
    before = h.d.qmax_stats()
    assert h.step(batches[N_GROWN])[0] and not h.m.pending
    after = h.d.qmax_stats()
    assert after[:2] == (41, 40 * N + N_GROWN)
    for k in (2, 3):                                  # the totals go on from where they were, by this step's own pairs
        assert before[k] + 200 * N_GROWN <= after[k] <= before[k] + 254 * N_GROWN, (k, before, after)
    last = after
    seen = []
    for _ in range(70):
        seen.append(h.step(batches[N_GROWN])[0])
        now = h.d.qmax_stats()
        assert now[2] >= last[2] and now[3] >= last[3]
        last = now
    assert seen == [True] * 55 + [False] * 15         # the copy of S = 64 is evaluated behind S = 96
    assert h.d.qmax_guard() == (1, HOLD_STEPS - 15) and h.m.decisions == [(96, 64, True)]
    h.close("growth while a copy is pending")


def test_explicit_request_during_the_hold(xq, batches, degenerate):
    """xq_dqn_set_qmax_mode(SCREENED) in the middle of a hold: screening resumes at once, and the next decision — on a net that has
    been made benign — counts nothing from before the hold."""
    from cn_chess_ai_amd import _capi
    batch = batches[N]
    h = Handle(xq, degenerate)
    run_to_first_fallback(h, batch)
    assert not any(h.run(batch, 25))
    h.d.set_params(h.w, h.b, net=TARGET)
    h.d.set_qmax_mode(_capi.QMAX_SCREENED)
    h.m.set_mode_screened()
    assert h.d.qmax_guard() == (1, 0)
    assert h.run(batch, 200) == [True] * 200
    assert h.d.qmax_guard() == (1, 0) and h.m.decisions[1:] == [(128, 96, False), (192, 160, False), (256, 224, False)]
    h.close("explicit request during the hold")
