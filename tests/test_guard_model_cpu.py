"""tests/guard_model.py on synthetic counter streams: the step numbers the header comment of xq_dqn_set_qmax_mode documents, and the
negative control — the same model without "a decision never counts a step that ran before the end of the last hold" shows the spurious
second fallback that tests/test_guard_lifecycle_gpu.py asserts against.  No device."""
import pytest

from guard_model import CHECK_EVERY, HOLD_STEPS, GuardModel, counter_blocks

N = 1024
BENIGN = (3 * N, N // 50)                    # candidate pairs, whole groups a screened step of a harmless net adds: 3 and 0.02 per sample
DEGENERATE = (250 * N, 220 * N)              # every output ties: 250 of the 254 groups per sample, most of them whole


class Stream:
    """a handle asked to screen every TD step: the device counts only the steps that do screen"""

    def __init__(self, model, per_step=BENIGN, n=N):
        self.m, self.per_step, self.n = model, per_step, n
        self.totals = [0, 0]
        self.td_steps = 0
        self.screened = []                    # TD step numbers (1-based) that screened

    def run(self, steps):
        out = []
        for _ in range(steps):
            self.td_steps += 1
            s = self.m.tick(self.n)
            if s:
                self.totals[0] += self.per_step[0] * self.n // N
                self.totals[1] += self.per_step[1] * self.n // N
                self.m.queue(self.n, self.totals)
                self.screened.append(self.td_steps)
            out.append((s, self.m.fallbacks, self.m.hold))
        return out


def test_counter_blocks():
    assert (counter_blocks(1), counter_blocks(512), counter_blocks(1024), counter_blocks(1025), counter_blocks(1100)) == (16, 16, 32, 48, 48)


def test_a_benign_net_never_falls_back():
    s = Stream(GuardModel())
    out = s.run(3000)
    assert all(o == (True, 0, 0) for o in out)
    assert s.m.steps == 3000 and s.m.samples == 3000 * N and not s.m.stage_whole
    # one decision per 64 screened steps, each on the copy queued 32 steps before it
    assert [d[:2] for d in s.m.decisions[:3]] == [(64, 32), (128, 96), (192, 160)] and not any(d[2] for d in s.m.decisions)


def test_a_degenerate_net_falls_back_at_the_documented_steps():
    """TD steps 1..64 screen, 65..576 run the full product, 577..640 screen (S = 65..128), 641..1152 full, ...: 64 + 512 per cycle"""
    s = Stream(GuardModel(), DEGENERATE)
    out = s.run(3 * (2 * CHECK_EVERY + HOLD_STEPS) + 10)
    cycle = 2 * CHECK_EVERY + HOLD_STEPS
    for t, (screened, fallbacks, hold) in enumerate(out, start=1):
        k, r = divmod(t - 1, cycle)                  # r = 0..63: screened steps of cycle k; r = 64..575: its hold
        assert screened == (r < 2 * CHECK_EVERY), t
        assert fallbacks == k + (r >= 2 * CHECK_EVERY), t
        assert hold == (cycle - 1 - r if r >= 2 * CHECK_EVERY else 0), t
    assert out[64] == (False, 1, 511) and out[575] == (False, 1, 0) and out[576] == (True, 1, 0) and out[640] == (False, 2, 511)
    assert s.m.stage_whole
    # the second decision's copy was queued behind S = 96 and its window starts behind S = 65, the first screened step after the hold
    assert s.m.decisions[:2] == [(64, 32, True), (128, 96, True)]


def degenerate_then_benign(model, switch_at=300, after=400):
    s = Stream(model, DEGENERATE)
    s.run(switch_at)                                  # falls back at TD step 65; the net changes in the middle of the hold
    s.per_step = BENIGN
    s.run(2 * CHECK_EVERY + HOLD_STEPS - switch_at)
    assert (s.m.fallbacks, s.m.hold) == (1, 0) and s.td_steps == 576
    return s, s.run(after)


def test_a_net_made_benign_during_the_hold_is_not_held_again():
    s, out = degenerate_then_benign(GuardModel())
    assert all(o == (True, 1, 0) for o in out)
    assert s.m.decisions == [(64, 32, True), (128, 96, False), (192, 160, False), (256, 224, False), (320, 288, False), (384, 352, False),
                             (448, 416, False)]
    assert not s.m.stage_whole                        # ... and the staged pass is switched off again by the first clean window


def test_control_without_the_rule_the_second_fallback_is_spurious():
    """the library as it was: the window of the second decision reaches back to S = 33..64, from before the hold"""
    s, out = degenerate_then_benign(GuardModel(rebase_after_hold=False))
    first_held = next(i for i, o in enumerate(out) if not o[0])
    assert first_held == 64                           # S = 65..128 screen, then TD step 641 is held although the net has been benign for 340 steps
    assert out[first_held] == (False, 2, 511)
    assert s.m.decisions[1] == (128, 96, True)


@pytest.mark.parametrize("rule,fallbacks", [(True, 1), (False, 2)])
def test_a_window_holds_no_step_from_before_the_hold(rule, fallbacks):
    """a benign net at 23 pairs per sample passes (limit 24) only if NOT ONE of the degenerate steps is in its window: with one of 250 in
    a window of 31 steps the mean is 30"""
    m = GuardModel(rebase_after_hold=rule)
    s = Stream(m, DEGENERATE)
    s.run(100)
    s.per_step = (23 * N, 0)
    s.run(2 * CHECK_EVERY + HOLD_STEPS - 100 + 300)
    assert m.fallbacks == fallbacks


@pytest.mark.parametrize("rule,fallbacks", [(True, 1), (False, 2)])
def test_an_explicit_request_during_the_hold_screens_at_once_and_the_next_decision_is_clean(rule, fallbacks):
    m = GuardModel(rebase_after_hold=rule)
    s = Stream(m, DEGENERATE)
    out = s.run(90)
    assert out[-1] == (False, 1, HOLD_STEPS - 26)
    s.per_step = BENIGN
    m.set_mode_screened()
    out = s.run(200)
    assert out[0] == (True, 1, 0)
    assert m.fallbacks == fallbacks
    if rule:
        assert all(o == (True, 1, 0) for o in out) and m.decisions[1] == (128, 96, False)


def test_growth_drops_the_pending_copy_and_the_net_is_still_caught():
    m = GuardModel()
    s = Stream(m, DEGENERATE)
    s.run(40)
    assert m.pending and m.queued_at == 32
    s.n = 1100                                        # 48 counter pairs instead of 32
    out = s.run(1)
    assert out == [(True, 0, 0)] and not m.pending
    out = s.run(60)
    # the next copy is that of S = 64, evaluated behind S = 96 on the window since the start: TD step 97 is the first held one
    assert all(o == (True, 0, 0) for o in out[:55]) and out[55] == (False, 1, 511)
    assert m.decisions == [(96, 64, True)]


def test_growth_that_drops_the_rebasing_copy_queues_it_again():
    s, _ = degenerate_then_benign(GuardModel(), after=5)          # S = 65 queued the re-basing copy
    m = s.m
    assert m.pending and m.rebase and m.queued_at == 65
    s.n = 1100
    s.run(1)
    assert m.pending and m.rebase and m.queued_at == 70           # dropped at the top of the step, queued again behind it
    out = s.run(300)
    assert all(o == (True, 1, 0) for o in out) and m.decisions[1] == (128, 96, False)
