"""Arena — player A against player B over P pairs of games, all 2P games at once on the GPU (include/xq_capi.h, xq_arena).

Games [0, P) have A as Red, games [P, 2P) have A as Black; twins g and g + P play the same random opening with the seats
swapped (DESIGN.md §4 "Arena").  A player is a DQN, a Search (the fixed material search of DESIGN.md §4 "Search player") or None
(uniform-random play).  The summary is computed here, on the host, from the per-game records.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import call, ArenaGame, ARENA_LIVE, ARENA_GENERAL_CAPTURED, ARENA_NO_LEGAL_MOVE, ARENA_MOVE_CAP, ARENA_OPENING
from .vecenv import VecEnv, STEP_DTYPE, _ptr

GAME_DTYPE = np.dtype([("cause", "u1"), ("winner", "u1"), ("a_result", "i1"), ("a_is_red", "u1"), ("plies", "<u2"),
                       ("red_score", "<i2"), ("black_score", "<i2"), ("reserved", "<u2")])
assert GAME_DTYPE.itemsize == C.sizeof(ArenaGame)
CAUSES = {ARENA_LIVE: "live", ARENA_GENERAL_CAPTURED: "general_captured", ARENA_NO_LEGAL_MOVE: "no_legal_move",
          ARENA_MOVE_CAP: "move_cap", ARENA_OPENING: "opening"}


def summarize(records, n_pairs):
    """Score of A from the records: wins / draws / losses over the games outside the opening, s = (W + D/2) / N, a 95 % interval
    from the variance of the PAIR scores (twins are correlated), and the Elo difference -400 log10(1/s - 1), clamped at s = 0, 1."""
    r = np.asarray(records)
    res = r["a_result"].astype(np.int64)
    scored = (r["cause"] != ARENA_LIVE) & (r["cause"] != ARENA_OPENING)
    w, d, l = (int(np.sum(scored & (res == k))) for k in (1, 0, -1))
    n = w + d + l
    out = dict(games=int(len(r)), pairs=int(n_pairs), wins=w, draws=d, losses=l, scored_games=n,
               causes={name: int(np.sum(r["cause"] == c)) for c, name in CAUSES.items()})
    if n == 0:
        out.update(score=float("nan"), ci95=(float("nan"), float("nan")), elo=float("nan"), scored_pairs=0)
        return out
    s = (w + 0.5 * d) / n
    pair_ok = scored[:n_pairs] & scored[n_pairs:]
    pts = (res + 1) / 2.0
    pair_score = (pts[:n_pairs] + pts[n_pairs:])[pair_ok] / 2.0
    m = len(pair_score)
    half = 1.96 * math.sqrt(float(np.var(pair_score, ddof=1)) / m) if m > 1 else float("inf")
    sc = min(max(s, 0.5 / n), 1.0 - 0.5 / n)                # clamp: an all-win (or all-loss) run gives a finite Elo
    out.update(score=s, ci95=(max(0.0, s - half), min(1.0, s + half)), elo=-400.0 * math.log10(1.0 / sc - 1.0), scored_pairs=m)
    return out


class Search:
    """The material search player: a full-width negamax of `depth` (1, 2 or 3) plies, exploring with probability eps."""

    def __init__(self, depth, eps=0.0):
        if int(depth) != depth or not 1 <= depth <= 3:
            raise ValueError(f"Search depth must be 1, 2 or 3 (got {depth!r})")
        if not 0.0 <= float(eps) <= 1.0:
            raise ValueError(f"Search eps must be in [0, 1] (got {eps!r})")
        self.depth, self.eps = int(depth), float(eps)

    def __repr__(self):
        return f"Search({self.depth}, eps={self.eps})"


def player(p, eps=0.0):
    """The _capi.ArenaPlayer of None (uniform-random play), a Search, or a DQN that explores with eps."""
    if p is None:
        return _capi.ArenaPlayer(_capi.PLAYER_RANDOM, None, 0, 0.0)
    if isinstance(p, Search):
        return _capi.ArenaPlayer(_capi.PLAYER_SEARCH, None, p.depth, p.eps)
    return _capi.ArenaPlayer(_capi.PLAYER_NET, p.handle, 0, float(eps))


class Arena:
    def __init__(self, n_pairs, seed=0x5EED, first_game_id=0, stream=None, opening_plies=8):
        self.n_pairs = int(n_pairs)
        h = C.c_void_p()
        call("xq_arena_create", self.n_pairs, int(seed), int(first_game_id), stream, C.byref(h))
        self._h = h
        e = C.c_void_p()
        call("xq_arena_env", self._h, C.byref(e))
        self.env = VecEnv(0, _handle=e)          # borrowed view of the arena's games
        self.reset(opening_plies)

    def close(self):
        if self._h is not None:
            call("xq_arena_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reset(self, opening_plies=8):
        call("xq_arena_reset", self._h, int(opening_plies))

    def set_temperature(self, temp_a=0.0, temp_b=0.0):
        """A Boltzmann temperature per player (DESIGN.md §4 "Exploration policy"), 0 = greedy, else in [1e-3, 1e3]: network players and
        caller-supplied rows draw their non-epsilon plies from the softmax of the legal moves' values; random and search players and
        the opening are untouched.  Survives reset()."""
        call("xq_arena_set_temperature", self._h, float(temp_a), float(temp_b))

    def temperature(self):
        a, b = C.c_double(), C.c_double()
        call("xq_arena_get_temperature", self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def ply_q_dev(self, q_dev, q_stride=96, eps_a=0.0, eps_b=0.0, view_a=False, view_b=False):
        """One ply with caller Q rows: q_dev = device pointer (int) or a cuda torch tensor [2P][>= 90], None = random.  view_a / view_b:
        that player's rows are in the mover's view (computed on view_boards' boards)."""
        if hasattr(q_dev, "data_ptr"):
            q_stride = int(q_dev.stride(0))
            q_dev = q_dev.data_ptr()
        if view_a or view_b:
            call("xq_arena_ply_q_dev_view", self._h, q_dev, int(q_stride), float(eps_a), float(eps_b), int(bool(view_a)), int(bool(view_b)))
            return
        call("xq_arena_ply_q_dev", self._h, q_dev, int(q_stride), float(eps_a), float(eps_b))

    def run(self, dqn_a, dqn_b, eps_a=0.0, eps_b=0.0, max_plies=0):
        """Plays until every game has ended (or max_plies plies); dqn_* = DQN, Search or None (uniform random).  eps_a / eps_b are
        the networks' exploration (a Search carries its own).  -> plies played."""
        n = C.c_int32()
        if isinstance(dqn_a, Search) or isinstance(dqn_b, Search):
            pa, pb = player(dqn_a, eps_a), player(dqn_b, eps_b)
            call("xq_arena_run_players", self._h, C.byref(pa), C.byref(pb), int(max_plies), C.byref(n))
            return n.value
        call("xq_arena_run", self._h, dqn_a.handle if dqn_a is not None else None,
             dqn_b.handle if dqn_b is not None else None, float(eps_a), float(eps_b), int(max_plies), C.byref(n))
        return n.value

    def results(self):
        rec = np.zeros(2 * self.n_pairs, dtype=GAME_DTYPE)
        call("xq_arena_results", self._h, rec.ctypes.data_as(C.POINTER(ArenaGame)))
        return rec

    def live(self):
        n = C.c_int32()
        call("xq_arena_live", self._h, C.byref(n))
        return n.value

    def last_step(self):
        res = np.zeros(2 * self.n_pairs, dtype=STEP_DTYPE)
        call("xq_arena_last_step", self._h, res.ctypes.data_as(C.POINTER(_capi.StepResult)))
        return res

    def summary(self):
        return summarize(self.results(), self.n_pairs)
