"""Reference of the reward rule (include/xq_capi.h, xq_env_set_reward; DESIGN.md §4 "Reward rule"): the formula in np.float32, the
material balance B and its change delta computed FROM THE TWO BOARDS of a transition (so nothing here leans on anybody's capture
bookkeeping), the argument rules, a deliberately wrong formula (negative control), oracle replays of self-play, and versus_ref.Collect
with the reward replaced.  No device, no library: the GPU tests compare the rings the env kernel writes with these."""
import numpy as np

import versus_ref as vr
import xqoracle as xo

EVALUATE, DELTA = 0, 1
# PieceScore by piece code (chessboard.h:23-31): 1..7 Red general, advisor, elephant, horse, chariot, cannon, soldier; 8..14 Black
VALUE = np.array([0, 1000, 20, 20, 40, 90, 45, 10, 1000, 20, 20, 40, 90, 45, 10], dtype=np.int64)
TYPES = ("general", "advisor", "elephant", "horse", "chariot", "cannon", "soldier")
DEFAULTS = (1e-3, 0.0, 1.0)


def balance(board, side):
    """B(board, side): the PieceScore sum of side's pieces minus the other side's (side 0 Red, 1 Black)"""
    b = np.asarray(board).astype(np.int64)
    red = int(VALUE[b[(b >= 1) & (b <= 7)]].sum())
    black = int(VALUE[b[b >= 8]].sum())
    return red - black if side == 0 else black - red


def delta(s, s2, side):
    """the change of side's material balance from board s to board s2"""
    return balance(s2, side) - balance(s, side)


def formula(d, scale, ply_cost, bound):
    """r = min(max(fl32(fl32((float)d * s32) - c32), -b32), b32), one rounding per operation"""
    s32, c32, b32 = np.float32(scale), np.float32(ply_cost), np.float32(bound)
    prod = np.float32(np.float32(d) * s32)
    r = np.float32(prod - c32)
    return np.float32(min(max(r, np.float32(-b32)), b32))


def formula_fused(d, scale, ply_cost, bound):
    """NEGATIVE CONTROL: the product and the difference rounded once together, as one fused multiply-add gives them.  d * s32 is exact in
    fp64 (11 x 24 bits) and so is the difference for the magnitudes used here, so the one rounding is the conversion to fp32."""
    s32, c32, b32 = np.float32(scale), np.float32(ply_cost), np.float32(bound)
    r = np.float32(np.float64(d) * np.float64(s32) - np.float64(c32))
    return np.float32(min(max(r, np.float32(-b32)), b32))


def formula_fp64(d, scale, ply_cost, bound):
    """the same expression on the fp32 parameters in fp64, not rounded"""
    s, c, b = float(np.float32(scale)), float(np.float32(ply_cost)), float(np.float32(bound))
    return min(max(d * s - c, -b), b)


def args_ok(kind, scale, ply_cost, bound):
    """xq_env_set_reward's argument rules, on the fp32 values: a known kind, scale finite > 0, ply_cost finite >= 0, bound > 0 or +inf"""
    with np.errstate(over="ignore"):
        s, c, b = np.float32(scale), np.float32(ply_cost), np.float32(bound)
    return bool(kind in (EVALUATE, DELTA) and np.isfinite(s) and s > 0 and np.isfinite(c) and c >= 0 and b > 0)


def mover_of(s2, action_to):
    """the side that moved in a self-play transition: the colour of the piece now standing on the move's target square"""
    return 0 if s2[action_to] <= 7 else 1


def ring_reward(s, action_to, s2, params, side=None):
    """the delta-rule reward of one stored transition from its own boards; side None: self-play (the mover's balance).  A row without an
    action is an empty row: its boards are equal and delta = 0."""
    if action_to < 0:
        d = 0
    else:
        d = delta(s, s2, mover_of(s2, action_to) if side is None else side)
    return formula(d, *params)


class SelfPlay:
    """Self-play on the CPU oracle in lockstep with a VecEnv: n games, game g on Philox stream first_id + g, ply counter as the env
    kernel's (it counts the plies played and survives a reset)."""

    def __init__(self, n, seed, first_id):
        self.n, self.seed, self.first = n, seed, first_id
        self.boards = [xo.new_board() for _ in range(n)]
        self.plies = [0] * n
        self.victims = {}                        # piece type 1..7 -> captures seen

    def step(self, q=None, eps=0.0):
        """one ply everywhere -> per game (s, action_to, captured value, mover, s' before any reset, evaluateBoard reward, done)"""
        out = []
        for g, b in enumerate(self.boards):
            s, mover = b.squares(), b.currentPlayer
            codes, _ = xo.all_valid_actions(b, mover)
            o = xo.selfplay_step(b, None if q is None else q[g], self.seed, self.first + g, self.plies[g], xo.eps_to_u32(eps))
            if o.action_code < 0:
                out.append((s, -1, 0, mover, s, int(o.reward), int(o.done)))
                continue
            self.plies[g] += 1
            f, to = divmod(int(o.action_code), 90)
            victim = int(s[to])
            s2 = s.copy()
            s2[to], s2[f] = s[f], 0
            if victim:
                t = (victim - 1) % 7 + 1
                self.victims[t] = self.victims.get(t, 0) + 1
            out.append((s, to, int(VALUE[victim]), mover, s2, int(o.reward), int(o.done)))
        return out


class DeltaCollect(vr.Collect):
    """versus_ref.Collect with the delta rule: the reward of a transition is formula(B(s', learner) - B(s, learner)) over the boards the
    slot itself gets — s = the board in front of the learner's half-ply, s' = the board as the collect leaves it (before any reset)."""

    def __init__(self, seed, learner_eps, opp, params):
        super().__init__(seed, learner_eps, opp)
        self.params = params
        # per written transition: (game id, delta, what the learner took, what the reply took, movePiece's own score change over it)
        self.deltas = []

    def phase_b(self, game, q_row):
        game.before_b = None if game.written else game.b.squares()
        game.score_b = game.b.redScore + game.b.blackScore          # movePiece's own bookkeeping, for the CPU cross-check
        game.after_b = None
        super().phase_b(game, q_row)
        if not game.written:
            game.after_b = game.b.squares()

    def reward(self, game):
        s = game.pending[0] if game.pending is not None else game.before_b
        s2 = game.b.squares()
        d = delta(s, s2, game.learner)
        mid = game.after_b if game.pending is not None else s2
        took, lost = delta(s, mid, game.learner), -delta(mid, s2, game.learner)
        assert d == took - lost and took >= 0 and lost >= 0
        self.deltas.append((game.gid, d, took, lost, game.b.redScore + game.b.blackScore - game.score_b))
        return formula(d, *self.params)


def versus_run(n, collects, seed, first, opp, params, learner_eps=1.0, q_learner=None):
    """`collects` versus collects of n fresh games -> (slots of every collect, all (gid, delta, took, lost, scored), all results)"""
    games = [vr.Game(first + g) for g in range(n)]
    slots, deltas, results = [], [], []
    for _ in range(collects):
        c = DeltaCollect(seed, learner_eps, opp, params)
        slots.append(c.run(games, q_learner))
        deltas += c.deltas
        results += c.results
    return slots, deltas, results
