"""The screening guard of xq_dqn_set_qmax_mode (include/xq_capi.h) as plain Python: no library import, no device.

The rule, in screened-step counts S (a TD step that runs the full product does not count):
  * behind every screened step with S % 32 == 0 the candidate counters are copied back, unless a copy is still pending;
  * a pending copy is evaluated at the top of the first TD step at which S % 32 == 0 again and S is not the S it was queued at — one
    window late.  Its window is everything between the totals of the last evaluation (`seen`) and the copy's own totals;
  * more than 24 candidate pairs or more than 1 whole group per sample of the window: that TD step and the 511 behind it run the full
    product (`hold`), `fallbacks` counts it.  Whole groups per sample above 0.25 switch `stage_whole` on, below 0.10 off;
  * A DECISION NEVER COUNTS A STEP THAT RAN BEFORE THE END OF THE LAST HOLD: when a hold begins, `seen` is marked stale (`rebase`).
    The first screened step behind the hold — however the hold ended, by running out or by an explicit set_qmax_mode — queues a
    copy at once, whatever S is; that copy decides nothing: at the next S % 32 == 0 it becomes `seen`, and the ordinary copy of that
    boundary is queued behind it;
  * a larger batch that needs a larger counter array drops the pending copy (the totals are carried over); a dropped re-basing copy
    is queued again behind the next screened step.

So for a net the screen cannot handle, asked to screen every step: S = 1..64 screen, TD steps 65..576 run the full product, S = 65..128
screen (copy behind S = 65 re-bases at S = 96; the copy of S = 96, window S = 66..96, is evaluated behind S = 128), TD steps 641..1152
run the full product, and so on: every cycle is 64 screened steps and 512 full ones.

`rebase_after_hold=False` is the rule WITHOUT the capitalised sentence (the library before it was added): the negative control."""

CHECK_EVERY = 32
HOLD_STEPS = 512
MAX_PAIRS = 24.0             # candidate (sample, group) pairs per sample
MAX_WHOLE = 1.0              # pairs recomputed as whole groups per sample
STAGE_ON, STAGE_OFF = 0.25, 0.10
REFINE_SAMPLES = 32          # samples per refine block = per counter pair
SAMPLE_PAD = 512             # the sample dimension of the screen's buffers is padded to this


def counter_blocks(n):
    """counter pairs a batch of n samples needs (n = 1024: 32, n = 1100: 48)"""
    return (n + SAMPLE_PAD - 1) // SAMPLE_PAD * SAMPLE_PAD // REFINE_SAMPLES


class GuardModel:
    def __init__(self, rebase_after_hold=True):
        self.rebase_after_hold = rebase_after_hold
        self.steps = 0                       # screened steps
        self.samples = 0
        self.pending = False
        self.queued_at = 0
        self.queued_samples = 0
        self.queued_totals = (0, 0)          # what the pending copy will read: the device's totals behind the step it was queued at
        self.seen = [0, 0, 0]                # samples, pairs, whole groups at the last evaluation (or re-base)
        self.rebase = False                  # a hold began and `seen` has not been re-based since
        self.hold = 0
        self.fallbacks = 0
        self.stage_whole = False
        self.blocks = 0
        self.decisions = []                  # (S at the evaluation, S its copy was queued at, fell back?) for the tests' messages

    def set_mode_screened(self):
        """an explicit xq_dqn_set_qmax_mode(SCREENED): the screen is on again at once"""
        self.hold = 0

    def _decide(self):
        ds = self.queued_samples - self.seen[0]
        dp, dw = self.queued_totals[0] - self.seen[1], self.queued_totals[1] - self.seen[2]
        fell = ds > 0 and (dp > MAX_PAIRS * ds or dw > MAX_WHOLE * ds)
        if fell:
            self.hold = HOLD_STEPS
            self.fallbacks += 1
            self.rebase = self.rebase_after_hold
        if ds > 0:
            share = dw / ds
            if share > STAGE_ON:
                self.stage_whole = True
            elif share < STAGE_OFF:
                self.stage_whole = False
        self.decisions.append((self.steps, self.queued_at, fell))
        self.seen = [self.queued_samples, self.queued_totals[0], self.queued_totals[1]]

    def tick(self, n):
        """top of a TD step of n samples that asks for the screen -> whether it screens"""
        blocks = counter_blocks(n)
        if blocks > self.blocks:                     # the counter array is replaced: its totals are carried, a pending copy is dropped
            if self.blocks:
                self.pending = False
            self.blocks = blocks
        if self.pending and not self.rebase and self.steps % CHECK_EVERY == 0 and self.steps != self.queued_at:
            self.pending = False
            self._decide()
        screened = self.hold == 0
        if self.hold > 0:
            self.hold -= 1
        return screened

    def queue(self, n, totals):
        """behind a screened step; totals = (pairs, whole groups) the device reports behind it, cumulative"""
        self.steps += 1
        self.samples += n
        boundary = self.steps % CHECK_EVERY == 0
        if self.rebase and self.pending and boundary:        # the re-basing copy: decides nothing
            self.pending = False
            self.rebase = False
            self.seen = [self.queued_samples, self.queued_totals[0], self.queued_totals[1]]
        if (boundary or self.rebase) and not self.pending:
            self.pending = True
            self.queued_at, self.queued_samples, self.queued_totals = self.steps, self.samples, (int(totals[0]), int(totals[1]))

    def step(self, n, totals):
        """one TD step whose cumulative device totals BEHIND it are `totals` (unchanged ones if it did not screen)
        -> (screened, fallbacks, hold_left) as xq_dqn_qmax_stats / xq_dqn_qmax_guard show them behind the step"""
        screened = self.tick(n)
        if screened:
            self.queue(n, totals)
        return screened, self.fallbacks, self.hold
