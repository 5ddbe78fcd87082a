"""Versus training (DESIGN.md §4 "Versus training") restated on the CPU oracle: one collect of a trainer that plays a fixed opponent,
over xqoracle (all_valid_actions, xqo_move_piece, xqo_evaluate_board, philox) and search_ref.arena_pick.

Per game, in order: (a) the opponent's pre-move where it is to move (a game it ends there gives an empty slot and sits out the collect),
(b) the learner's epsilon-greedy half-ply, (c) the opponent's reply unless (b) ended the game.  The transition runs from the board
before (b) to the board after (c); reward = evaluateBoard(learner, moveCount) there.  The Q rows of either side come from callables
that take the list of boards (the device test feeds the device's own Q values; the hand-built positions feed fixed rows).
"""
import ctypes as C

import numpy as np

import search_ref as sr
import xqoracle as xo

RED, BLACK = 0, 1
RANDOM, NET, SEARCH = 0, 1, 2
NO_PAIRS = 1 << 40          # arena_pick's twin stream with more pairs than games: the game's own stream


class Opponent:
    """kind RANDOM, NET (q: boards -> [n][>=90] rows) or SEARCH (depth); eps as the arena's players."""

    def __init__(self, kind, eps=0.0, depth=0, q=None):
        self.kind, self.eps, self.depth, self.q = kind, float(eps), int(depth), q


class Game:
    def __init__(self, gid, board=None, plies=0, episodes=0):
        self.gid = gid                            # first_game_id + g
        self.b = board if board is not None else xo.new_board()
        self.plies, self.episodes = plies, episodes
        self.written = False                      # this collect's slot is complete (the game sits out the later phases)
        self.slot = None                          # (s, action_to, reward, done, s') of the last collect
        self.pending = None                       # (s, action_to) between (b) and (c)

    @property
    def learner(self):
        return self.gid & 1


def _eps_greedy(codes, q_row, r, eps_u32):
    """<SELFPLAY>'s select: explore iff r0 < eps_u32 (codes[r1 % n]), else the first maximum of Q[to] (NaN never wins)."""
    n = len(codes)
    if q_row is None or r[0] < eps_u32:
        return int(codes[r[1] % n])
    best, top = 0, -np.inf
    for k, c in enumerate(codes):
        v = np.float32(q_row[int(c) % 90])
        if v == v and v > top:
            best, top = k, v
    return int(codes[best])


def pick(game, side, seed, q_row, eps, opp=None):
    """The code the mover plays (None: no legal move).  opp = None: the learner's epsilon-greedy on q_row."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    codes, _ = xo.all_valid_actions(game.b, side)
    if len(codes) == 0:
        return None
    r = xo.philox([game.plies, 0, game.gid, 0], key)
    if opp is None or opp.kind == NET:
        return _eps_greedy(codes, q_row, r, xo.eps_to_u32(eps))
    if opp.kind == RANDOM:
        return int(codes[r[1] % len(codes)])
    return sr.arena_pick(game.b, side, opp.depth, seed, game.gid, 0, NO_PAIRS, game.plies, opp.eps)


def _generals(b):
    sq = b.squares()
    return bool((sq == 1).any()), bool((sq == 8).any())


class Collect:
    """One versus collect over `games`; records the episode records and the per-game outcomes it produced."""

    def __init__(self, seed, learner_eps, opp):
        self.seed, self.eps, self.opp = seed, learner_eps, opp
        self.episodes = []                        # (game_id, episode, red_score, black_score, move_count, winner, no_action)
        self.results = []                         # (game_id, +1 win / 0 draw / -1 loss) from the learner's side

    def _half_ply(self, game, q_row, learner_moves):
        """Plays one half-ply of the side to move; -> (code or None, ended, no_action)."""
        b = game.b
        side = b.currentPlayer
        code = pick(game, side, self.seed, q_row, self.eps if learner_moves else self.opp.eps, None if learner_moves else self.opp)
        if code is None:
            return None, True, True
        f, t = divmod(code, 90)
        xo.lib().xqo_move_piece(C.byref(b), f // 9, f % 9, t // 9, t % 9)
        game.plies += 1
        return code, bool(xo.lib().xqo_check_game_over(C.byref(b))), False

    def _end(self, game, no_action, mover):
        b = game.b
        red_g, black_g = _generals(b)
        if not (red_g and black_g):
            res = 1 if (RED if red_g else BLACK) == game.learner else -1       # the captor wins
        elif no_action:
            res = -1 if mover == game.learner else 1                           # the side to move loses
        else:
            res = 0                                                            # the 200-move cap
        self.results.append((game.gid, res))
        self.episodes.append((game.gid, game.episodes + 1, b.redScore, b.blackScore, b.moveCount,
                              int(xo.lib().xqo_get_winner(C.byref(b))), int(no_action)))
        game.b = xo.new_board()
        game.episodes += 1

    def reward(self, game):
        return int(xo.lib().xqo_evaluate_board(C.byref(game.b), game.learner, game.b.moveCount))

    def phase_a(self, game, q_row=None):
        game.written, game.pending = False, None
        if game.b.currentPlayer == game.learner:
            return
        mover = game.b.currentPlayer
        _, ended, no_action = self._half_ply(game, q_row, False)
        if ended:
            s = game.b.squares()
            game.slot = (s, -1, 0, 1, s)
            self._end(game, no_action, mover)
            game.written = True

    def phase_b(self, game, q_row):
        if game.written:
            return
        s = game.b.squares()
        mover = game.b.currentPlayer
        code, ended, no_action = self._half_ply(game, q_row, True)
        to = -1 if code is None else code % 90
        if ended:
            game.slot = (s, to, self.reward(game), 1, game.b.squares())
            self._end(game, no_action, mover)
            game.written = True
        else:
            game.pending = (s, to)

    def phase_c(self, game, q_row=None):
        if game.written:
            game.written = False
            return
        mover = game.b.currentPlayer
        _, ended, no_action = self._half_ply(game, q_row, False)
        done = ended or game.b.moveCount + 1 >= 200
        s, to = game.pending
        game.slot = (s, to, self.reward(game), int(done), game.b.squares())
        game.pending = None
        if ended:
            self._end(game, no_action, mover)

    def run(self, games, q_learner, q_opp=None):
        """The whole collect: each phase over every game, the Q rows of a phase from the boards as that phase finds them."""
        def rows(fn):
            return fn([g.b for g in games]) if fn is not None else [None] * len(games)
        net = self.opp.kind == NET
        for g, q in zip(games, rows(self.opp.q if net else None)):
            self.phase_a(g, q)
        for g, q in zip(games, rows(q_learner)):
            self.phase_b(g, q)
        for g, q in zip(games, rows(self.opp.q if net else None)):
            self.phase_c(g, q)
        return [g.slot for g in games]
