"""VecEnv / ReplayBuffer — batched ChessBoard (reference include/chessboard.h:35-78) resident in HBM.

VecEnv is the build-defined batched form of the env half of ChessAI::train (reference chessai.cpp:90-119):
legal_moves() = getAllValidActions, step(actions) = movePiece + evaluateBoard + checkGameOver,
selfplay_step(q90, eps) = the whole ply on device with epsilon-greedy DQN::selectAction.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import StepResult, EpisodeRecord, call

RED, BLACK, NONE = 0, 1, 2

# reference chessboard.cpp:8-29
START_BOARD = np.zeros(90, dtype=np.uint8)
START_BOARD[0:9] = [5, 4, 3, 2, 1, 2, 3, 4, 5]
START_BOARD[81:90] = START_BOARD[0:9] + 7
START_BOARD[[19, 25]] = 6
START_BOARD[[64, 70]] = 13
START_BOARD[27:36:2] = 7
START_BOARD[54:63:2] = 14

STEP_DTYPE = np.dtype([("action", "<i4"), ("n_moves", "<i4"), ("reward", "<i4"), ("captured", "u1"), ("valid", "u1"),
                       ("done", "u1"), ("terminated", "u1"), ("winner", "u1"), ("explored", "u1"),
                       ("move_count", "<u2"), ("red_score", "<i2"), ("black_score", "<i2")])
EPISODE_DTYPE = np.dtype([("game_id", "<u4"), ("episode", "<u4"), ("red_score", "<i2"), ("black_score", "<i2"),
                          ("move_count", "<u2"), ("winner", "u1"), ("reserved", "u1")])
assert STEP_DTYPE.itemsize == 24 and EPISODE_DTYPE.itemsize == 16


def eps_to_u32(eps):
    """explore iff philox_word < eps_u32  (replaces `rand()/RAND_MAX < epsilon`, reference dqn.cpp:30-31)."""
    return int(min(max(float(eps), 0.0) * 4294967296.0, 4294967295.0))


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


REWARD_KINDS = {"evaluate": _capi.REWARD_EVALUATE, "delta": _capi.REWARD_DELTA}


def reward_kind(kind):
    """"evaluate" / "delta" -> XQ_REWARD_*; an int passes as it is (the library refuses an unknown one)."""
    if isinstance(kind, str):
        if kind not in REWARD_KINDS:
            raise ValueError(f"set_reward: expected 'evaluate' or 'delta', got {kind!r}")
        return REWARD_KINDS[kind]
    return int(kind)


POLICY_KINDS = {"greedy": _capi.POLICY_GREEDY, "boltzmann": _capi.POLICY_BOLTZMANN}


def policy_kind(kind):
    """"greedy" / "boltzmann" -> XQ_POLICY_*; an int passes as it is (the library refuses an unknown one)."""
    if isinstance(kind, str):
        if kind not in POLICY_KINDS:
            raise ValueError(f"set_policy: expected 'greedy' or 'boltzmann', got {kind!r}")
        return POLICY_KINDS[kind]
    return int(kind)


class ReplayBuffer:
    """ReplayBuffer{capacity; push(s,a,r,s',done); sample(B)} — element = the 5-tuple of DQN::train (dqn.cpp:157)."""

    def __init__(self, capacity, seed=0, stream=None, _handle=None):
        self._own = _handle is None
        if _handle is None:
            h = C.c_void_p()
            call("xq_replay_create", int(capacity), int(seed), stream, C.byref(h))
            _handle = h
        self._h = _handle

    def close(self):
        if self._h is not None and self._own:
            call("xq_replay_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def stream(self):
        """The HIP stream the ring runs on (its own when created without one), as an int."""
        s = C.c_void_p()
        call("xq_replay_stream", self._h, C.byref(s))
        return s.value

    def stats(self):
        size, cap, tot = C.c_int32(), C.c_int32(), C.c_uint64()
        call("xq_replay_size", self._h, C.byref(size), C.byref(cap), C.byref(tot))
        return size.value, cap.value, tot.value

    def __len__(self):
        return self.stats()[0]

    def track_next_player(self):
        """Make the ring record the side to move in every stored next board (what DQN.set_td_bootstrap("legal") reads).  While the
        ring is empty; afterwards push() needs next_player."""
        call("xq_replay_track_next_player", self._h)

    def next_player(self, first=0, n=None):
        """the side bytes of slots [first, first + n) of a tracking ring (0 = Red, 1 = Black)"""
        n = self.stats()[1] - first if n is None else n
        out = np.zeros(n, dtype=np.uint8)
        call("xq_replay_get_next_player", self._h, int(first), int(n), _ptr(out, C.c_uint8))
        return out

    def track_mover(self):
        """Make the ring record the side that moved in every stored board (what DQN.set_view("mover") reads, beside
        track_next_player()).  While the ring is empty; afterwards push() needs mover."""
        call("xq_replay_track_mover", self._h)

    def mover(self, first=0, n=None):
        """the who-moved bytes of slots [first, first + n) of a tracking ring (0 = Red, 1 = Black)"""
        n = self.stats()[1] - first if n is None else n
        out = np.zeros(n, dtype=np.uint8)
        call("xq_replay_get_mover", self._h, int(first), int(n), _ptr(out, C.c_uint8))
        return out

    def push(self, boards, action_to, reward, done, next_boards, next_player=None, mover=None):
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 90)
        next_boards = np.ascontiguousarray(next_boards, dtype=np.uint8).reshape(-1, 90)
        n = len(boards)
        a = np.ascontiguousarray(action_to, dtype=np.int32).reshape(n)
        r = np.ascontiguousarray(reward, dtype=np.float32).reshape(n)
        d = np.ascontiguousarray(done, dtype=np.uint8).reshape(n)
        if mover is not None:
            m = np.ascontiguousarray(mover, dtype=np.uint8).reshape(n)
            p = None if next_player is None else np.ascontiguousarray(next_player, dtype=np.uint8).reshape(n)
            call("xq_replay_push_host_sides", self._h, n, _ptr(boards, C.c_uint8), _ptr(a, C.c_int32), _ptr(r, C.c_float),
                 _ptr(d, C.c_uint8), _ptr(next_boards, C.c_uint8), _ptr(m, C.c_uint8), None if p is None else _ptr(p, C.c_uint8))
            return
        if next_player is not None:
            p = np.ascontiguousarray(next_player, dtype=np.uint8).reshape(n)
            call("xq_replay_push_host_sided", self._h, n, _ptr(boards, C.c_uint8), _ptr(a, C.c_int32), _ptr(r, C.c_float),
                 _ptr(d, C.c_uint8), _ptr(next_boards, C.c_uint8), _ptr(p, C.c_uint8))
            return
        call("xq_replay_push_host", self._h, n, _ptr(boards, C.c_uint8), _ptr(a, C.c_int32), _ptr(r, C.c_float),
             _ptr(d, C.c_uint8), _ptr(next_boards, C.c_uint8))

    def sample(self, batch, host=True):
        """host=False: the draw is only queued (no copy of the slots back, no synchronisation)."""
        if not host:
            call("xq_replay_sample", self._h, int(batch), None)
            return None
        slots = np.zeros(batch, dtype=np.int32)
        call("xq_replay_sample", self._h, int(batch), _ptr(slots, C.c_int32))
        return slots

    def sample_window(self, batch, start, count, host=True):
        """sample(B) from the `count` ring slots that start at `start` (wrapping)."""
        if not host:
            call("xq_replay_sample_window", self._h, int(batch), int(start), int(count), None)
            return None
        slots = np.zeros(batch, dtype=np.int32)
        call("xq_replay_sample_window", self._h, int(batch), int(start), int(count), _ptr(slots, C.c_int32))
        return slots

    # ---- prioritized replay (build-defined, BASELINE configs[4]) ----
    def enable_per(self, alpha=0.6, beta=0.4, eps=1e-3):
        call("xq_replay_enable_per", self._h, float(alpha), float(beta), float(eps))

    def per_rebuild(self, retire_start=0, retire_count=0, hold_start=0, hold_count=0):
        """hold: `hold_count` slots from `hold_start` count as priority 0 in the tree only (never drawn, not eligible); the live table
        keeps their values.  A hold of 0 is the plain rebuild."""
        if hold_count == 0 and hold_start == 0:
            call("xq_replay_per_rebuild", self._h, int(retire_start), int(retire_count))
        else:
            call("xq_replay_per_rebuild_hold", self._h, int(retire_start), int(retire_count), int(hold_start), int(hold_count))

    def sample_prioritized(self, batch, host=True):
        """(slots, normalised importance weights) of a stratified proportional draw from the tree as of the last rebuild."""
        if not host:
            call("xq_replay_sample_prioritized", self._h, int(batch), None, None)
            return None
        slots = np.zeros(batch, dtype=np.int32)
        w = np.zeros(batch, dtype=np.float32)
        call("xq_replay_sample_prioritized", self._h, int(batch), _ptr(slots, C.c_int32), _ptr(w, C.c_float))
        return slots, w

    def set_priorities(self, prio, first=0):
        p = np.ascontiguousarray(prio, dtype=np.float32)
        call("xq_replay_set_priorities", self._h, int(first), len(p), _ptr(p, C.c_float))

    def get_priorities(self, first=0, n=None):
        n = self.stats()[1] - first if n is None else n
        p = np.zeros(n, dtype=np.float32)
        call("xq_replay_get_priorities", self._h, int(first), int(n), _ptr(p, C.c_float))
        return p

    def per_stats(self):
        t, m, k = C.c_float(), C.c_float(), C.c_int32()
        call("xq_replay_per_stats", self._h, C.byref(t), C.byref(m), C.byref(k))
        return dict(total=t.value, max_priority=m.value, n_eligible=k.value)

    # ---- n-step TD returns (build-defined, DESIGN.md §4 "n-step returns") ----
    def set_n_step(self, n_step, stride=1):
        """Every DQN.td_grads_replay from this ring learns on n-step transitions: chains of n_step slots `stride` apart in age order
        (stride = the number of games whose collects fill the ring).  1 = off.  Takes effect at the next td_grads_replay."""
        call("xq_replay_set_n_step", self._h, int(n_step), int(stride))

    @property
    def n_step(self):
        """(n_step, stride) as last set; (1, 1) on a ring that was never asked."""
        n, s = C.c_int32(), C.c_int32()
        call("xq_replay_get_n_step", self._h, C.byref(n), C.byref(s))
        return n.value, s.value

    # ---- mirror augmentation (build-defined, DESIGN.md §4 "Mirror augmentation") ----
    def set_mirror(self, prob):
        """Every DQN.td_grads_replay from this ring reflects each minibatch row left-right (col -> 8 - col: both boards and the action)
        with probability prob, in a staged copy of the batch; the ring is never written.  0 = off.  NaN or a value outside [0, 1] is
        refused.  Takes effect at the next td_grads_replay."""
        call("xq_replay_set_mirror", self._h, float(prob))

    @property
    def mirror(self):
        """(prob, calls): prob as last set (0.0 on a ring that was never asked) and the number of mirror-mode TD steps queued from this
        ring so far — the call word of the next one's flag stream."""
        p, c = C.c_double(), C.c_uint64()
        call("xq_replay_get_mirror", self._h, C.byref(p), C.byref(c))
        return p.value, c.value

    # ---- colour-swap augmentation (build-defined, DESIGN.md §4 "Colour-swap augmentation") ----
    def set_colour_swap(self, prob):
        """Every DQN.td_grads_replay from this ring exchanges the colours of each minibatch row with probability prob (row -> 9 - row
        and Red <-> Black on both boards, the action's square, and 1 - side under the legal-move bootstrap), in a staged copy of the
        batch; the ring is never written.  0 = off.  NaN or a value outside [0, 1] is refused.  Takes effect at the next
        td_grads_replay; composes with set_mirror and set_n_step."""
        call("xq_replay_set_colour_swap", self._h, float(prob))

    def colour_swap(self):
        """(prob, calls): prob as last set (0.0 on a ring that was never asked) and the number of colour-swap-mode TD steps queued from
        this ring so far — the call word of the next one's flag stream (a counter of its own, apart from the mirror's)."""
        p, c = C.c_double(), C.c_uint64()
        call("xq_replay_get_colour_swap", self._h, C.byref(p), C.byref(c))
        return p.value, c.value

    def get(self, slot):
        b, nb = np.zeros(90, np.uint8), np.zeros(90, np.uint8)
        a, r, d = C.c_int32(), C.c_float(), C.c_uint8()
        call("xq_replay_get", self._h, int(slot), _ptr(b, C.c_uint8), C.byref(a), C.byref(r), C.byref(d),
             _ptr(nb, C.c_uint8))
        return b, a.value, r.value, d.value, nb


class VecEnv:
    def __init__(self, n_games, seed=0x5EED, first_game_id=0, stream=None, _handle=None):
        self._own = _handle is None
        if _handle is None:
            h = C.c_void_p()
            call("xq_env_create", int(n_games), int(seed), int(first_game_id), stream, C.byref(h))
            _handle = h
        self._h = _handle
        n = C.c_int32()
        call("xq_env_num_games", self._h, C.byref(n))
        self.n_games = n.value

    def close(self):
        if self._h is not None and self._own:
            call("xq_env_destroy", self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def stream(self):
        s = C.c_void_p()
        call("xq_env_stream", self._h, C.byref(s))
        return s.value

    def reset(self):
        call("xq_env_reset", self._h)

    def set_state(self, boards, meta=None, first=0):
        boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 90)
        n = len(boards)
        mp = None
        if meta is not None:
            meta = np.ascontiguousarray(meta, dtype=np.int32).reshape(n, 4)
            mp = _ptr(meta, C.c_int32)
        call("xq_env_set_state", self._h, int(first), n, _ptr(boards, C.c_uint8), mp)

    def get_state(self, first=0, n=None):
        n = self.n_games - first if n is None else n
        boards = np.zeros((n, 90), dtype=np.uint8)
        meta = np.zeros((n, 4), dtype=np.int32)
        call("xq_env_get_state", self._h, int(first), int(n), _ptr(boards, C.c_uint8), _ptr(meta, C.c_int32))
        return boards, meta

    def legal_moves(self, player=-1):
        """-> (codes [n][128] u16 in canonical order, counts [n])"""
        codes = np.zeros((self.n_games, _capi.MAX_MOVES), dtype=np.uint16)
        counts = np.zeros(self.n_games, dtype=np.int32)
        call("xq_env_legal_moves", self._h, int(player), _ptr(codes, C.c_uint16), _ptr(counts, C.c_int32))
        return codes, counts

    def search_values(self, depth):
        """Material search of every game for its side to move (DESIGN.md §4 "Search player"), depth 1..3 ->
        (values [n][128] int32 root value of each legal move in list order, INT32_MIN past the count; counts [n]; best [n] index of
        the first best move, -1 without a move)"""
        values = np.zeros((self.n_games, _capi.MAX_MOVES), dtype=np.int32)
        counts = np.zeros(self.n_games, dtype=np.int32)
        best = np.zeros(self.n_games, dtype=np.int32)
        call("xq_env_search", self._h, int(depth), _ptr(values, C.c_int32), _ptr(counts, C.c_int32), _ptr(best, C.c_int32))
        return values, counts, best

    def valid_matrix(self, game):
        m = np.zeros(8100, dtype=np.uint8)
        call("xq_env_valid_matrix", self._h, int(game), _ptr(m, C.c_uint8))
        return m

    def rule_matrix(self, game):
        """[7][8100] results of isValid{General..Soldier}Move (chessboard.h:50-56) for every in-board (from, to) of a game."""
        m = np.zeros((7, 8100), dtype=np.uint8)
        call("xq_env_rule_matrix", self._h, int(game), _ptr(m, C.c_uint8))
        return m

    def rule_query(self, game, piece_type, fr, fc, tr, tc):
        ok = C.c_int32()
        call("xq_env_rule_query", self._h, int(game), int(piece_type), int(fr), int(fc), int(tr), int(tc), C.byref(ok))
        return bool(ok.value)

    def get_winner(self, first=0, n=None):
        """ChessBoard::getWinner() per game (colour of the first general in index order)."""
        n = self.n_games - first if n is None else n
        w = np.zeros(n, dtype=np.uint8)
        call("xq_env_get_winner", self._h, int(first), int(n), _ptr(w, C.c_uint8))
        return w

    def step(self, actions, auto_reset=True):
        actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.n_games)
        res = np.zeros(self.n_games, dtype=STEP_DTYPE)
        call("xq_env_step", self._h, _ptr(actions, C.c_int32), int(bool(auto_reset)),
             res.ctypes.data_as(C.POINTER(StepResult)))
        return res

    def selfplay_step(self, q90=None, eps=0.1):
        """One ply everywhere.  q90: [n][90] float32 Q-values of outputs 0..89 (None = uniform random policy)."""
        res = np.zeros(self.n_games, dtype=STEP_DTYPE)
        qp = None
        if q90 is not None:
            q90 = np.ascontiguousarray(q90, dtype=np.float32).reshape(self.n_games, 90)
            qp = _ptr(q90, C.c_float)
        call("xq_env_selfplay_step_host", self._h, qp, eps_to_u32(eps), res.ctypes.data_as(C.POINTER(StepResult)))
        return res

    def selfplay_step_dev(self, q90_dev=0, q_stride=96, eps=0.1, results_dev=None, replay=None):
        """Asynchronous, device pointers only (ints): the hot-loop form."""
        call("xq_env_selfplay_step", self._h, C.c_void_p(q90_dev) if q90_dev else None, int(q_stride), eps_to_u32(eps),
             C.c_void_p(results_dev) if results_dev else None, replay.handle if replay is not None else None)

    # ---- mover view (build-defined, DESIGN.md §4 "Mover view") ----
    def set_q_view(self, on=True):
        """The Q rows handed to selfplay_step / selfplay_step_dev from now on are in the mover's view (DQN.set_view("mover"), built from
        view_boards): with Black to move the greedy pick reads q[swap(to)] for the destination `to`.  Nothing else of the step
        changes."""
        if not isinstance(on, (bool, int)) or on not in (0, 1):
            raise ValueError(f"set_q_view: expected a bool, got {on!r}")
        call("xq_env_set_q_view", self._h, 1 if on else 0)

    @property
    def q_view(self):
        v = C.c_int32()
        call("xq_env_get_q_view", self._h, C.byref(v))
        return bool(v.value)

    # ---- reward rule (build-defined, DESIGN.md §4 "Reward rule") ----
    def set_reward(self, kind, scale=1e-3, ply_cost=0.0, bound=1.0):
        """What the env kernel writes into a replay ring as the reward: "evaluate" = evaluateBoard as the reference (the default), or
        "delta" = clamp(fl32(fl32(delta * scale) - ply_cost), -bound, bound) in fp32, delta = the change of the mover's (versus: the
        learner's) material balance over the transition.  scale finite > 0, ply_cost finite >= 0, bound > 0 (inf: no clamp).  Takes
        effect at the next ply that writes a ring; the reward field of a step result stays evaluateBoard."""
        call("xq_env_set_reward", self._h, reward_kind(kind), float(scale), float(ply_cost), float(bound))

    @property
    def reward(self):
        """(kind, scale, ply_cost, bound) as last set; ("evaluate", 1e-3, 0.0, 1.0) on an env that was never asked."""
        k, s, c, b = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        call("xq_env_get_reward", self._h, C.byref(k), C.byref(s), C.byref(c), C.byref(b))
        names = {v: n for n, v in REWARD_KINDS.items()}
        return names[k.value], s.value, c.value, b.value

    # ---- exploration policy (build-defined, DESIGN.md §4 "Exploration policy") ----
    def set_policy(self, kind, temperature=1.0):
        """How a ply that reads Q rows and did not take the epsilon branch picks: "greedy" = the first maximum (the default), or
        "boltzmann" = a softmax draw over the legal moves' values at `temperature` in [1e-3, 1e3] (tests/boltzmann_ref.py is the rule).
        Takes effect at the next selfplay_step*; a step result's `explored` is 2 where the draw left the first maximum."""
        call("xq_env_set_policy", self._h, policy_kind(kind), float(temperature))

    def policy(self):
        """(kind, temperature) as last set; ("greedy", 1.0) on an env that was never asked."""
        k, t = C.c_int32(), C.c_double()
        call("xq_env_get_policy", self._h, C.byref(k), C.byref(t))
        names = {v: n for n, v in POLICY_KINDS.items()}
        return names[k.value], t.value

    def drain_episodes(self, max_records=65536):
        rec = np.zeros(max_records, dtype=EPISODE_DTYPE)
        n, total = C.c_int32(), C.c_uint64()
        call("xq_env_drain_episodes", self._h, rec.ctypes.data_as(C.POINTER(EpisodeRecord)), int(max_records),
             C.byref(n), C.byref(total))
        return rec[:n.value], total.value

    def counters(self):
        c = (C.c_uint64 * 6)()
        call("xq_env_counters", self._h, c)
        return dict(zip(("plies", "episodes", "red_wins", "black_wins", "captures", "explored"), [int(x) for x in c]))

    def boards_dev(self):
        return _capi.load().xq_env_boards_dev(self._h)
