"""Versus training (DESIGN.md §4 "Versus training") without a device: the CPU restatement of one collect on hand-built positions, the
facade probe compiled with plain g++, and the Python argument checks of Trainer.set_opponent that need no trainer."""
import ctypes as C
import os

import numpy as np
import pytest

import versus_ref as vr
import xqoracle as xo

from test_arena_cpu import gxx, BUILD, ROOT

RED, BLACK = 0, 1
G, A, E, H, R, CN, S = 1, 2, 3, 4, 5, 6, 7      # Red codes; Black = code + 7
SEED = 0x5EED


def sq(r, c):
    return r * 9 + c


def code(f, t):
    return sq(*f) * 90 + sq(*t)


def position(pieces, player, move_count=0):
    b = np.zeros(90, dtype=np.uint8)
    for (r, c), p in pieces.items():
        b[sq(r, c)] = p
    return xo.board_from(b, move_count, player)


def one_row(to, size=96):
    q = np.zeros(size, dtype=np.float32)
    q[to] = 1.0
    return q


def run(game, opp, q_learner=None, eps=0.0):
    c = vr.Collect(SEED, eps, opp)
    slot = c.run([game], (lambda boards: [q_learner]) if q_learner is not None else (lambda boards: [None]))[0]
    return c, slot


def evaluate(squares, color, move_count):
    b = xo.board_from(squares, move_count, 0)
    return int(xo.lib().xqo_evaluate_board(C.byref(b), color, move_count))


def build_versus_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "versus_facade.cpp"), os.path.join(BUILD, "versus_facade"))


def test_learner_black_at_reset_waits_for_the_opponent():
    g = vr.Game(gid=7)                                   # odd id: the learner plays Black
    assert g.learner == BLACK
    start = g.b.squares()
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.RANDOM), eps=1.0)
    # s is the start position after Red's pre-move: one Red piece moved, Black (the learner) to move
    assert (s != start).sum() == 2 and done == 0
    codes, _ = xo.all_valid_actions(xo.board_from(s, 1, BLACK), BLACK)
    assert to in {int(x) % 90 for x in codes}
    assert g.b.moveCount == 3 and g.b.currentPlayer == BLACK and g.plies == 3
    assert np.array_equal(s2, g.b.squares())
    assert r == evaluate(s2, BLACK, 3)
    assert c.results == [] and c.episodes == []
    # an even id plays Red: no pre-move, two half-plies
    h = vr.Game(gid=8)
    run(h, vr.Opponent(vr.RANDOM), eps=1.0)
    assert h.b.moveCount == 2 and h.b.currentPlayer == RED


def test_learner_captures_the_general():
    g = vr.Game(gid=2, board=position({(0, 4): G, (9, 4): G + 7, (5, 4): R, (9, 0): R + 7}, RED, 10))
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.SEARCH, depth=1), one_row(sq(9, 4)))
    assert to == sq(9, 4) and done == 1
    assert s2[sq(9, 4)] == R and r == evaluate(s2, RED, 11) == 998
    assert c.results == [(2, 1)]
    assert c.episodes[0][:2] == (2, 1) and c.episodes[0][5] == RED and c.episodes[0][6] == 0
    assert np.array_equal(g.b.squares(), xo.new_board().squares()) and g.episodes == 1 and g.plies == 1


def test_opponent_captures_the_general_in_its_reply():
    # the Black chariot faces the Red general down an open file; the learner (Red) pushes a soldier instead
    g = vr.Game(gid=4, board=position({(0, 3): G, (9, 4): G + 7, (6, 3): R + 7, (6, 8): S}, RED, 40))
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.SEARCH, depth=1), one_row(sq(7, 8)))
    assert to == sq(7, 8) and done == 1
    assert s2[sq(0, 3)] == R + 7 and (s2 == G).sum() == 0
    assert r == evaluate(s2, RED, 42) and r < -1000               # the learner's view of the board the reply left
    assert c.results == [(4, -1)] and c.episodes[0][5] == BLACK
    assert g.written is False and g.b.moveCount == 0


def test_learner_without_a_move_loses():
    # Black (the learner, odd id) to move with no piece left: no action, s' = s, the slot closes the game
    g = vr.Game(gid=3, board=position({(0, 4): G, (4, 4): R}, BLACK, 20))
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.RANDOM), one_row(0))
    assert to == -1 and done == 1 and np.array_equal(s, s2)
    assert r == evaluate(s, BLACK, 20)
    assert c.results == [(3, -1)] and c.episodes[0][6] == 1
    assert g.plies == 0 and g.episodes == 1


def test_opponent_without_a_move_in_the_pre_move_gives_an_empty_slot():
    g = vr.Game(gid=6, board=position({(0, 4): G, (4, 4): R}, BLACK, 20))     # Red learner, Black (no piece) to move
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.SEARCH, depth=2), one_row(0))
    assert (to, r, done) == (-1, 0, 1) and np.array_equal(s, s2)
    assert s[sq(4, 4)] == R                                        # the board as the pre-move left it (before the reset)
    assert c.results == [(6, 1)]
    # the game sat out the rest of the collect: reset, nobody moved, the reply phase cleared the mark
    assert np.array_equal(g.b.squares(), xo.new_board().squares()) and g.b.moveCount == 0 and not g.written


def test_transition_across_the_200_move_cap():
    pieces = {(0, 4): G, (9, 4): G + 7, (3, 0): R, (6, 8): R + 7}
    # moveCount 197, Red learner to move: (b) 198, (c) 199 -> done (moveCount + 1 >= 200) but the game goes on
    g = vr.Game(gid=0, board=position(pieces, RED, 197))
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.RANDOM), one_row(sq(4, 0)))
    assert done == 1 and g.b.moveCount == 199 and c.results == []
    assert r == evaluate(s2, RED, 199)
    # the next collect: the learner's half-ply reaches 200, the cap ends the game in (b): a draw, no reply
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.RANDOM), one_row(sq(5, 0)))
    assert done == 1 and c.results == [(0, 0)] and c.episodes[0][4] == 200
    assert r == evaluate(s2, RED, 200)
    assert g.b.moveCount == 0


def test_reward_is_the_learners_view():
    # the learner (Black) leaves its cannon en prise; the search reply takes it: the reward is Black's evaluation, negative
    pieces = {(0, 4): G, (9, 3): G + 7, (2, 8): R, (9, 8): CN + 7, (9, 0): S + 7}
    g = vr.Game(gid=1, board=position(pieces, BLACK, 30))
    c, (s, to, r, done, s2) = run(g, vr.Opponent(vr.SEARCH, depth=1), one_row(sq(8, 8)))
    assert to == sq(8, 8) and done == 0
    assert s2[sq(8, 8)] == R                                       # the chariot took the cannon
    assert r == evaluate(s2, BLACK, 32) == -83                     # (1010 - 1090) - 3.2, truncated; Red's view would be 76
    assert evaluate(s2, RED, 32) == 76


def test_net_opponent_is_epsilon_greedy_on_its_rows():
    g = vr.Game(gid=2, board=position({(0, 4): G, (9, 4): G + 7, (3, 0): R, (6, 8): R + 7}, RED, 0))
    q_opp = one_row(sq(6, 7))
    opp = vr.Opponent(vr.NET, eps=0.0, q=lambda boards: [q_opp] * len(boards))
    c, (s, to, r, done, s2) = run(g, opp, one_row(sq(4, 0)))
    assert s2[sq(6, 7)] == R + 7 and s2[sq(4, 0)] == R


def test_versus_facade_probe_compiles():
    assert os.path.exists(build_versus_facade_probe())


def test_set_opponent_rejects_other_players():
    from cn_chess_ai_amd import Trainer

    class Fake(Trainer):
        def __init__(self):
            self._h = None
    with pytest.raises(TypeError):
        Fake().set_opponent("search-1")
    with pytest.raises(TypeError):
        Fake().set_opponent(3)
