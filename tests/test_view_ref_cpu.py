"""CPU checks of the mover view (not gpu): tests/view_ref.py against tests/colour_swap_ref.py with the flags taken from the sides, on
the 730 boards of tests/golden/ref_sparse.npz; why the step refuses colour-swap augmentation under the view (the view of a swapped
transition is the view of the transition); the oracle's legal-move sets through the view; and a negative control: flagging s' by the
mover instead of by the next side is told apart on every self-play row."""
import ctypes as C
import os

import numpy as np
import pytest

import colour_swap_ref as cr
import view_ref as vr
import xqoracle as xo


@pytest.fixture(scope="module")
def sparse(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_sparse.npz"))["board"].astype(np.uint8)


@pytest.fixture(scope="module")
def selfplay_rows(sparse):
    """one self-play transition per board and side that has a move: (s, to of the side's k-th legal move, s', mover, next side)"""
    L = xo.lib()
    S, A, S2, M = [], [], [], []
    for i, b in enumerate(sparse):
        for side in (0, 1):
            codes, n = xo.all_valid_actions(xo.board_from(b, player=side), side)
            if n == 0:
                continue
            f, t = divmod(int(codes[i % n]), 90)
            p = xo.board_from(b, player=side)
            L.xqo_move_piece(C.byref(p), f // 9, f % 9, t // 9, t % 9)
            S.append(b); A.append(t); S2.append(np.array(p.squares(), np.uint8)); M.append(side)
    S, S2 = np.array(S, np.uint8), np.array(S2, np.uint8)
    A, M = np.array(A, np.int32), np.array(M, np.uint8)
    return dict(S=S, A=A, S2=S2, mover=M, next_player=(1 - M).astype(np.uint8))


def test_view_is_the_colour_swap_flagged_by_the_side(sparse):
    assert len(sparse) == 730
    for side in (0, 1):
        sides = np.full(len(sparse), side, np.uint8)
        want = cr.swap_board(sparse) if side else sparse
        assert np.array_equal(vr.view(sparse, sides), want)
    rng = np.random.default_rng(3)
    sides = rng.integers(0, 2, size=len(sparse)).astype(np.uint8)
    got = vr.view(sparse, sides)
    for b, s, g in zip(sparse, sides, got):                       # row by row, no masks
        assert np.array_equal(g, cr.swap_board(b) if s else b)
    a = rng.integers(-1, 96, size=len(sparse)).astype(np.int32)
    a[:8] = [-1, 0, 8, 81, 89, 90, 95, 44]
    ga = vr.view_action(a, sides)
    for x, s, g in zip(a, sides, ga):
        assert g == (int(cr.swap_action(x)) if s else x)
    assert ga.dtype == np.int32 and got.dtype == np.uint8
    # the 96-nibble form keeps nibbles 90..95 (which are 0)
    N = np.zeros((len(sparse), 96), np.uint8); N[:, :90] = sparse
    assert np.array_equal(vr.view(N, sides)[:, :90], got) and not vr.view(N, sides)[:, 90:].any()
    # a side byte is a flag: any non-zero value is Black
    assert np.array_equal(vr.view(sparse, sides * 7), got)


def test_apply_flags_the_two_boards_separately_and_stages_red_to_move(selfplay_rows):
    r = selfplay_rows
    out = vr.apply(r["S"], r["A"], r["S2"], r["mover"], r["next_player"])
    assert np.array_equal(out["flag_s"], r["mover"]) and np.array_equal(out["flag_next"], 1 - r["mover"])
    m = r["mover"].astype(bool)
    assert m.any() and (~m).any()
    assert np.array_equal(out["boards"][~m], r["S"][~m]) and np.array_equal(out["next_boards"][~m], cr.swap_board(r["S2"][~m]))
    assert np.array_equal(out["boards"][m], cr.swap_board(r["S"][m])) and np.array_equal(out["next_boards"][m], r["S2"][m])
    assert np.array_equal(out["action"][m], cr.swap_action(r["A"][m])) and np.array_equal(out["action"][~m], r["A"][~m])
    assert not out["next_player"].any()
    # versus rows: both flags are the learner's colour
    vs = vr.apply(r["S"], r["A"], r["S2"], r["mover"], r["mover"])
    assert np.array_equal(vs["next_boards"][m], cr.swap_board(r["S2"][m])) and np.array_equal(vs["next_boards"][~m], r["S2"][~m])
    fx = dict(S=r["S"], A=r["A"], S2=r["S2"])
    slots = np.random.default_rng(4).integers(0, len(m), size=300)
    st = vr.stage(fx, slots, r["mover"], r["next_player"])
    assert np.array_equal(st["slot"], slots) and np.array_equal(st["boards"], out["boards"][slots])
    assert np.array_equal(st["next_boards"], out["next_boards"][slots]) and np.array_equal(st["action"], out["action"][slots])


def test_view_of_a_swapped_transition_is_the_view_of_the_transition(selfplay_rows):
    """why xq_dqn_td_grads_replay refuses colour-swap augmentation under the view: swap exchanges the colours AND the sides, so the view
    undoes it, on every nibble and action"""
    r = selfplay_rows
    for nxt in (r["next_player"], r["mover"]):                    # self-play rows and versus rows
        plain = vr.apply(r["S"], r["A"], r["S2"], r["mover"], nxt)
        swapped = vr.apply(cr.swap_board(r["S"]), cr.swap_action(r["A"]), cr.swap_board(r["S2"]), 1 - r["mover"], 1 - nxt)
        for k in ("boards", "next_boards", "action", "next_player"):
            assert np.array_equal(plain[k], swapped[k]), k
        assert np.array_equal(swapped["flag_s"], 1 - plain["flag_s"]) and np.array_equal(swapped["flag_next"], 1 - plain["flag_next"])
    odd = np.array([-1, 90, 95, 8099], np.int32)                  # actions outside the board stay what they are either way
    for side in (0, 1):
        s = np.full(4, side, np.uint8)
        assert np.array_equal(vr.view_action(cr.swap_action(odd), 1 - s), vr.view_action(odd, s))


def swap_code(code):
    f, t = divmod(int(code), 90)
    return int(cr.swap_action(f)) * 90 + int(cr.swap_action(t))


def test_reds_moves_on_the_view_are_the_image_of_the_sides_moves(sparse):
    """against the oracle: the legal-move SET of Red on view(b, side) is the image of side's set on b (what lets the staged side byte of a
    legal-bootstrap step be 0 on every row, and the pick read q[swap(to)])"""
    compared = moves = 0
    for b in sparse:
        for side in (0, 1):
            codes, n = xo.all_valid_actions(xo.board_from(b, player=side), side)
            v = vr.view(b[None], np.array([side], np.uint8))[0]
            vcodes, vn = xo.all_valid_actions(xo.board_from(v, player=0), 0)
            assert n <= xo.MAX_MOVES and vn == n
            image = [swap_code(c) if side else int(c) for c in codes]
            assert sorted(image) == sorted(int(c) for c in vcodes)
            # ... and the destinations, which is all the net's outputs index
            assert sorted(c % 90 for c in image) == sorted(int(vr.view_action([int(c) % 90], [side])[0]) for c in codes)
            compared += 1
            moves += n
    assert compared == 1460 and moves == 30157


def test_flagging_the_next_board_by_the_mover_is_detected_on_every_selfplay_row(selfplay_rows):
    """negative control: in self-play the side to move in s' is the other side, so a transform that used the mover's flag for both boards
    (the colour-swap kernel's one flag) stages another s' on every row"""
    r = selfplay_rows
    right = vr.apply(r["S"], r["A"], r["S2"], r["mover"], r["next_player"])
    wrong = vr.apply(r["S"], r["A"], r["S2"], r["mover"], r["mover"])
    assert len(r["A"]) > 1400
    assert (right["next_boards"] != wrong["next_boards"]).any(axis=1).all()
    assert np.array_equal(right["boards"], wrong["boards"]) and np.array_equal(right["action"], wrong["action"])
    # ... and Red's moves on the wrongly flagged s' are not the next side's moves
    differ = samples = 0
    for s2, p, w in list(zip(r["S2"], r["next_player"], wrong["next_boards"]))[::10]:
        samples += 1
        codes, n = xo.all_valid_actions(xo.board_from(s2, player=int(p)), int(p))
        wcodes, wn = xo.all_valid_actions(xo.board_from(w, player=0), 0)
        image = sorted(swap_code(c) if p else int(c) for c in codes)
        differ += image != sorted(int(c) for c in wcodes)
    print("wrongly flagged s' with other moves: %d of %d" % (differ, samples))
    assert 2 * differ > samples


def test_pick_rows_permutes_black_rows_only():
    rng = np.random.default_rng(5)
    q = rng.standard_normal((6, 90)).astype(np.float32)
    side = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    qb = vr.pick_rows(q, side)
    for g in range(6):
        for t in range(90):
            assert qb[g, int(cr.swap_action(t)) if side[g] else t] == q[g, t]
