"""cn_chess_ai_amd/csrc/xq_l0hot.h — the table that says which rows of gW0^T the layer-0 gradient computes on the matrix pipe ("hot") and
which it sums from occurrence lists ("cold") — printed by tests/cpp/l0hot_probe.cpp (plain g++) and checked here:
  * the packing is a bijection: every one of the 1260 rows is exactly one packed hot row or exactly one cold row, both maps invert, the
    per-square masks and cold bases say the same, a group's rows lie on its own run of at most 32 squares;
  * the hot set holds every (square, piece) of every position under tests/golden/;
  * the hot set holds the closure computed independently: one piece alone on the oracle's board, moved by the oracle's move generator
    (oracle/xq_oracle.c) from its start squares until nothing new appears.
No result of the library depends on the table (tests/test_l0_hot_grad_gpu.py puts pieces on cold rows); what these checks protect is the
speed of positions from play, which must never take the cold route."""
import os

import numpy as np
import pytest

import xqoracle as xo
from l0_hot_ref import COLD_BIT, NO_ROW, load_table


@pytest.fixture(scope="module")
def table():
    return load_table()


def hot_rows(t):
    return set(int(r) for r in t["row"] if r != NO_ROW)


def test_packing_is_a_bijection_on_the_1260_rows(table):
    t = table
    row, index, cold_row = t["row"], t["index"], t["cold_row"]
    assert len(row) == t["groups"] * t["group_rows"] and t["groups"] * t["group_rows"] // 16 <= 48
    hot = [int(r) for r in row if r != NO_ROW]
    cold = [int(r) for r in cold_row[:t["n_cold"]]]
    assert len(hot) == t["n_hot"] and len(set(hot)) == len(hot) and len(set(cold)) == len(cold)
    assert np.all(cold_row[t["n_cold"]:] == NO_ROW) and cold == sorted(cold)
    assert not set(hot) & set(cold) and set(hot) | set(cold) == set(range(1260))
    for r in range(1260):
        i = int(index[r])
        if i & COLD_BIT:
            assert cold_row[i & ~COLD_BIT] == r
        else:
            assert row[i] == r
    for g in range(t["groups"]):
        lo, hi = int(t["sq0"][g]), int(t["sq0"][g + 1])
        assert 0 <= hi - lo <= t["sq_b"]
        rows = row[g * t["group_rows"]:(g + 1) * t["group_rows"]]
        live = rows[rows != NO_ROW]
        assert np.all(rows[:len(live)] == live) and np.all(np.diff(live) > 0)          # padding behind the rows, rows ascending
        assert np.all((live // 14 >= lo) & (live // 14 < hi))
    assert t["sq0"][0] == 0 and t["sq0"][t["groups"]] == 90
    for s in range(90):
        planes = [p for p in range(14) if (int(t["hot_mask"][s]) >> p) & 1]
        assert set(s * 14 + p for p in planes) == set(r for r in hot if r // 14 == s)
        assert t["cold_base"][s] == sum(1 for r in cold if r // 14 < s)


def test_hot_set_holds_every_piece_of_every_golden_position(table, golden_dir):
    hot = hot_rows(table)
    seen = 0
    for name in sorted(os.listdir(golden_dir)):
        if not name.endswith(".npz"):
            continue
        z = np.load(os.path.join(golden_dir, name))
        for key in z.files:
            boards = z[key]
            if boards.ndim != 2 or boards.shape[1] != 90 or boards.dtype != np.uint8:      # (every array of boards is [positions][90] u8)
                continue
            sq = np.nonzero(boards)
            rows = set((sq[1] * 14 + boards[sq].astype(np.int64) - 1).tolist())
            assert rows <= hot, (name, key, sorted(rows - hot))
            seen += len(boards)
    assert seen > 6000


def test_hot_set_holds_the_closure_of_the_oracles_move_generator(table):
    hot = hot_rows(table)
    start = xo.new_board().squares()
    closure = set()
    for code in range(1, 15):
        reached = set(int(s) for s in np.nonzero(start == code)[0])
        frontier = list(reached)
        assert frontier
        while frontier:
            s = frontier.pop()
            sq = np.zeros(90, dtype=np.uint8)
            sq[s] = code
            moves, n = xo.all_valid_actions(xo.board_from(sq), 0 if code <= 7 else 1)
            assert n == len(moves)
            for m in moves:
                assert int(m) // 90 == s
                if int(m) % 90 not in reached:
                    reached.add(int(m) % 90)
                    frontier.append(int(m) % 90)
        closure |= set(s * 14 + code - 1 for s in reached)
    assert len(closure) > 600 and closure <= hot, sorted(closure - hot)
    # and the table holds nothing else: with no blockers on the board the two closures are the same set
    assert hot == closure
