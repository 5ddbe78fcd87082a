"""The search player (DESIGN.md §4 "Search player") restated on the CPU oracle: a full-width negamax over
xqoracle.all_valid_actions (the env's move list, capped at 128), moves played with xqo_move_piece.

    N(pos, side, k, d) = -(MATE - k)                     if side has no move
                       = max over moves m of child(m)   otherwise
    child(m) = MATE - (k + 1)                            if m captures a general
             = c                                         if d == 1
             = c - N(pos o m, other side, k + 1, d - 1)  otherwise,   c = value of the piece on m.to (0 if empty)

The root values of a position are child(m) for every root move, k = 0, d = depth.  The arena pick draws like the env kernel.
"""
import ctypes as C

import xqoracle as xo

MATE = 1000000
PIECE_VALUE = (0, 1000, 20, 20, 40, 90, 45, 10)      # PieceScore by type, chessboard.h:23-31


def _value(code):
    return PIECE_VALUE[code - 7 if code > 7 else code]


def _child(b, side, k, d, code):
    f, t = divmod(int(code), 90)
    victim = b.sq[t]
    if victim == 1 or victim == 8:
        return MATE - (k + 1)
    c = _value(victim)
    if d == 1:
        return c
    saved = (b.sq[f], b.moveCount, b.currentPlayer, b.redScore, b.blackScore)
    xo.lib().xqo_move_piece(C.byref(b), f // 9, f % 9, t // 9, t % 9)
    v = c - negamax(b, 1 - side, k + 1, d - 1)
    b.sq[f], b.sq[t] = saved[0], victim
    b.moveCount, b.currentPlayer, b.redScore, b.blackScore = saved[1:]
    return v


def negamax(b, side, k, d):
    """N(pos, side, k, d) of the board b (an xqoracle.Board, restored on return)."""
    codes, _ = xo.all_valid_actions(b, side)
    if len(codes) == 0:
        return -(MATE - k)
    return max(_child(b, side, k, d, c) for c in codes)


def root_values(b, side, depth):
    """-> (codes, [child(m) for every root move m]) with k = 0, d = depth."""
    codes, _ = xo.all_valid_actions(b, side)
    return codes, [_child(b, side, 0, depth, c) for c in codes]


def position(squares, player, move_count=0, red=0, black=0):
    return xo.board_from(squares, move_count, player, red, black)


def arena_pick(b, side, depth, seed, first_game_id, g, pairs, ply, eps):
    """The action code the search player plays in arena game g at ply `ply` (outside the opening), None without a move.
    Exploring (r0 < eps_u32 on ctr {ply, 0, first_game_id + g, 0}) takes codes[r1 % n]; otherwise one of the best root moves, the
    (r0 % n_best)-th in list order with r drawn on the pair's stream ctr {ply, 0, first_game_id + g mod pairs, 3}."""
    key = [seed & 0xFFFFFFFF, seed >> 32]
    codes, _ = xo.all_valid_actions(b, side)
    if len(codes) == 0:
        return None
    r = xo.philox([ply, 0, first_game_id + g, 0], key)
    if r[0] < xo.eps_to_u32(eps):
        return int(codes[r[1] % len(codes)])
    _, vals = root_values(b, side, depth)
    top = max(vals)
    best = [i for i, v in enumerate(vals) if v == top]
    t = xo.philox([ply, 0, first_game_id + g % pairs, 3], key)
    return int(codes[best[t[0] % len(best)]])
