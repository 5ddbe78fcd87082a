"""Seeded board generators of the sparse-position tests (tests/test_rules_sparse_gpu.py, tests/test_rules_negative_control_cpu.py):
(a) legal-looking endgames, (b) line stress for chariots and cannons, (c) arbitrary placements, (d) no piece of the side to move.
Plain helper: no GPU, no oracle."""
import itertools
import random

import numpy as np

VALUE = np.array([0, 1000, 20, 20, 40, 90, 45, 10, 1000, 20, 20, 40, 90, 45, 10], dtype=np.int64)


def _squares_by_type():
    """[side][type] -> the squares a piece of that type can stand on in a game from the start position"""
    out = [[None] * 8 for _ in range(2)]
    for side in (0, 1):
        m = (lambda s: s) if side == 0 else (lambda s: 89 - s)          # Black = Red turned by 180 degrees
        out[side][1] = [m(r * 9 + c) for r in range(3) for c in (3, 4, 5)]
        out[side][2] = [m(s) for s in (3, 5, 13, 21, 23)]
        out[side][3] = [m(s) for s in (2, 6, 18, 22, 26, 38, 42)]
        out[side][4] = out[side][5] = out[side][6] = list(range(90))
        out[side][7] = [m(r * 9 + c) for r in (3, 4) for c in (0, 2, 4, 6, 8)] + [m(s) for s in range(45, 90)]
    return out


def gen_endgames(n, seed):
    """class (a) -> (boards [n][90], meta [n][4]); half the boards carry scores that explain the material (tracked)"""
    rnd = random.Random(seed)
    where = _squares_by_type()
    bag = [2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 7, 7, 7]
    boards = np.zeros((n, 90), dtype=np.uint8)
    meta = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        b = [0] * 90
        for side in (0, 1):
            k = rnd.randint(1, 6)
            types = ([1] if rnd.random() < 0.875 else []) + rnd.sample(bag, k - 1)
            for t in types[:k]:
                for _ in range(4):
                    s = rnd.choice(where[side][t])
                    if b[s] == 0:
                        b[s] = t + 7 * side
                        break
        boards[i] = b
        meta[i, 0] = rnd.randrange(200)
        meta[i, 1] = rnd.randrange(2)
    mat_red = (VALUE[boards] * (boards <= 7)).sum(axis=1)
    mat_black = (VALUE[boards] * (boards >= 8)).sum(axis=1)
    tracked = np.arange(n) % 2 == 0
    meta[:, 2] = np.where(tracked, 1480 - mat_black, 0)
    meta[:, 3] = np.where(tracked, 1480 - mat_red, 0)
    return boards, meta


def gen_line_stress(seed):
    """class (b): every (row or column, index on it, chariot / cannon, colour) x every set of 0-3 other occupied squares of that line
    and the full line; variant 0 bare, variant 1 with up to 4 pieces elsewhere."""
    rnd = random.Random(seed)
    lines = [[r * 9 + c for c in range(9)] for r in range(10)] + [[r * 9 + c for r in range(10)] for c in range(9)]
    out_b, out_m = [], []
    for line in lines:
        for pos in range(len(line)):
            others = [s for k, s in enumerate(line) if k != pos]
            sets = [c for k in range(4) for c in itertools.combinations(others, k)] + [tuple(others)]
            for occupied in sets:
                for piece in (5, 6, 12, 13):
                    for variant in (0, 1):
                        b = [0] * 90
                        b[line[pos]] = piece
                        for s in occupied:
                            b[s] = rnd.randint(1, 14)
                        if variant:
                            for _ in range(rnd.randint(1, 4)):
                                s = rnd.randrange(90)
                                if s not in line:
                                    b[s] = rnd.randint(1, 14)
                        out_b.append(b)
                        out_m.append((rnd.randrange(200), int(piece > 7) if variant == 0 else rnd.randrange(2),
                                      rnd.choice((0, 0, 90, 1000)), rnd.choice((0, 0, 45, 1480))))
    return np.array(out_b, dtype=np.uint8), np.array(out_m, dtype=np.int32)


def gen_arbitrary(n, seed, empty_mover=False):
    """class (c): 0-16 pieces a side of any type on any square; class (d) (empty_mover): the side to move has none."""
    rnd = random.Random(seed)
    boards = np.zeros((n, 90), dtype=np.uint8)
    meta = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        player = rnd.randrange(2)
        k = [rnd.randint(0, 16), rnd.randint(0, 16)]
        if empty_mover:
            k[player] = 0
            if i % 64 == 0:
                k = [0, 0]                                              # the empty board
        sq = rnd.sample(range(90), k[0] + k[1])
        for j, s in enumerate(sq):
            boards[i, s] = rnd.randint(1, 7) + (7 if j >= k[0] else 0)
        meta[i] = (rnd.randrange(200), player, rnd.choice((0, 10, 1000, 1480)), rnd.choice((0, 20, 1000, 1480)))
    return boards, meta
