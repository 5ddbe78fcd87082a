"""Search player (DESIGN.md §4 "Search player") without a device: the CPU restatement on hand-built positions, the facade probe and the
example compile with plain g++, and the Python player refuses depths outside 1..3."""
import os

import numpy as np
import pytest

import search_ref as sr
from cn_chess_ai_amd.arena import Search

from test_arena_cpu import gxx, BUILD, ROOT, build_example

RED, BLACK = 0, 1
G, A, E, H, R, C, S = 1, 2, 3, 4, 5, 6, 7      # Red codes; Black = code + 7


def sq(r, c):
    return r * 9 + c


def board(pieces):
    b = np.zeros(90, dtype=np.uint8)
    for (r, c), code in pieces.items():
        b[sq(r, c)] = code
    return b


def code(fr, to):
    return sq(*fr) * 90 + sq(*to)


def best_codes(codes, vals):
    top = max(vals)
    return top, {int(c) for c, v in zip(codes, vals) if v == top}


def build_search_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "search_facade.cpp"), os.path.join(BUILD, "search_facade"))


def test_depth1_takes_the_most_valuable_capture():
    # the Red chariot on (4,0) can take a cannon (45) along its row or a horse (40) along its column
    b = sr.position(board({(0, 4): G, (9, 5): G + 7, (4, 0): R, (4, 6): C + 7, (7, 0): H + 7}), RED)
    codes, vals = sr.root_values(b, RED, 1)
    top, best = best_codes(codes, vals)
    assert top == 45 and best == {code((4, 0), (4, 6))}
    assert vals[[int(c) for c in codes].index(code((4, 0), (7, 0)))] == 40
    assert sum(v != 0 for v in vals) == 2


def test_general_capture_beats_any_material():
    # the chariot on (9,0) reaches the Black general; the cannon could take a chariot (90) over a screen
    b = sr.position(board({(0, 4): G, (9, 4): G + 7, (9, 0): R, (2, 8): C, (5, 8): S + 7, (8, 8): R + 7}), RED)
    for depth in (1, 2, 3):
        codes, vals = sr.root_values(b, RED, depth)
        top, best = best_codes(codes, vals)
        assert top == sr.MATE - 1 and best == {code((9, 0), (9, 4))}, depth
        assert vals[[int(c) for c in codes].index(code((2, 8), (8, 8)))] < sr.MATE - 1


def test_depth2_keeps_its_general_out_of_reach():
    # the Black chariot on (7,4) faces the Red general on (1,4); the horse could grab a soldier (10) instead of stepping aside
    b = sr.position(board({(1, 4): G, (9, 3): G + 7, (7, 4): R + 7, (3, 1): H, (5, 2): S + 7}), RED)
    grab = code((3, 1), (5, 2))
    codes, vals = sr.root_values(b, RED, 1)
    assert best_codes(codes, vals)[1] == {grab}
    codes, vals = sr.root_values(b, RED, 2)
    c = [int(x) for x in codes]
    assert vals[c.index(grab)] == 10 - (sr.MATE - 2)
    top, best = best_codes(codes, vals)
    assert top == 0 and grab not in best and code((1, 4), (1, 3)) in best


def test_depth2_keeps_its_chariot_out_of_reach():
    # taking the soldier on (4,8) puts the Red chariot in front of the Black chariot on (8,8)
    b = sr.position(board({(0, 4): G, (9, 4): G + 7, (4, 0): R, (4, 8): S + 7, (8, 8): R + 7}), RED)
    grab = code((4, 0), (4, 8))
    codes, vals = sr.root_values(b, RED, 1)
    assert best_codes(codes, vals) == (10, {grab})
    codes, vals = sr.root_values(b, RED, 2)
    c = [int(x) for x in codes]
    assert vals[c.index(grab)] == 10 - 90
    assert vals[c.index(code((4, 0), (8, 0)))] == -90          # (8,0) lies on the Black chariot's row
    top, best = best_codes(codes, vals)
    assert top == 0 and grab not in best


def test_side_without_a_move_is_mated():
    only_red = board({(0, 4): G, (4, 4): R, (6, 4): S + 7})
    b = sr.position(only_red, BLACK)
    b.sq[sq(6, 4)] = 0
    for depth in (1, 2, 3):
        assert sr.negamax(b, BLACK, 0, depth) == -sr.MATE
    # Red takes Black's last piece: Black then has no move one ply below the root
    b = sr.position(only_red, RED)
    codes, vals = sr.root_values(b, RED, 2)
    assert vals[[int(x) for x in codes].index(code((4, 4), (6, 4)))] == 10 + sr.MATE - 1
    codes, vals = sr.root_values(b, RED, 1)
    assert max(vals) == 10


def test_search_player_rejects_other_depths():
    for bad in (0, 4, -1, 2.5):
        with pytest.raises(ValueError):
            Search(bad)
    with pytest.raises(ValueError):
        Search(2, eps=1.5)
    assert (Search(3, 0.25).depth, Search(3, 0.25).eps) == (3, 0.25)


def test_example_and_search_facade_compile_with_plain_gxx():
    assert os.path.exists(build_example())
    assert os.path.exists(build_search_facade_probe())
