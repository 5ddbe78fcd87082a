"""CPU checks of the colour-swap augmentation (not gpu): tests/colour_swap_ref.py's board map, action rule and flag rule; the symmetry
the feature rests on, on the oracle's rules engine over tests/golden/ref_sparse.npz (legal-move sets, movePiece, the scores,
evaluateBoard and checkGameOver all commute with the exchange of the colours under row -> 9 - row) with each half of the map alone told
apart; and header, ctypes table, library, work model and facade agreeing on the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import colour_swap_ref as cr
import xqoracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_replay_set_colour_swap", "xq_replay_get_colour_swap", "xq_dqn_last_colour_swap", "xq_trainer_set_colour_swap")
SEED = 0x5EED0123456789


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_swap_board_is_an_involution_square_by_square_and_on_the_words():
    rng = np.random.default_rng(1)
    B = rng.integers(0, 15, size=(200, 90)).astype(np.uint8)
    B[:15] = np.arange(15, dtype=np.uint8)[:, None]                           # every code on every square
    M = cr.swap_board(B)
    assert np.array_equal(cr.swap_board(M), B) and not np.array_equal(M, B)
    sigma = [0] + list(range(8, 15)) + list(range(1, 8))
    for r in range(10):
        for c in range(9):
            for code in range(15):
                assert M[code, (9 - r) * 9 + c] == sigma[code]
            assert np.array_equal(M[:, (9 - r) * 9 + c], np.array(sigma, np.uint8)[B[:, r * 9 + c]])
    assert (M == 0).sum() == (B == 0).sum() and np.array_equal((M >= 8), (cr.flip_rows(B) >= 1) & (cr.flip_rows(B) <= 7))
    # on the 96 nibbles of the packed layout: 90..95 stay where they are, and stay 0
    N = np.zeros((200, 96), np.uint8); N[:, :90] = B
    assert np.array_equal(cr.swap_board(N)[:, :90], M) and not cr.swap_board(N)[:, 90:].any()
    # the words: row r of the image is the 36 bits from bit 36 (9 - r) of the packed board with every nibble through sigma
    for b, m in zip(B[:30], M[:30]):
        wb, wm = cr.pack(b), cr.pack(m)
        vb, vm = sum(w << (32 * i) for i, w in enumerate(wb)), sum(w << (32 * i) for i, w in enumerate(wm))
        assert vm >> 360 == 0
        for r in range(10):
            row, mrow = (vb >> (36 * (9 - r))) & (2 ** 36 - 1), (vm >> (36 * r)) & (2 ** 36 - 1)
            assert [(mrow >> (4 * c)) & 15 for c in range(9)] == [sigma[(row >> (4 * c)) & 15] for c in range(9)]


def test_action_rule():
    got = cr.swap_action([-1, 0, 8, 81, 89, 90, 95, 8099])
    assert got.tolist() == [-1, 81, 89, 0, 8, 90, 95, 8099] and got.dtype == np.int32
    a = np.arange(90)
    m = cr.swap_action(a)
    assert np.array_equal(m // 9, 9 - a // 9) and np.array_equal(m % 9, a % 9) and np.array_equal(cr.swap_action(m), a)


def test_flag_rule():
    assert cr.flags(257, 1, 0, SEED).all() and cr.flags(257, 1.0, 7, SEED).dtype == np.uint8
    assert not cr.flags(257, 0.0, 0, SEED).any()
    rows = 4096
    per_call = [cr.flags(rows, 0.5, call, SEED) for call in range(4)]
    total = int(sum(int(f.sum()) for f in per_call))
    n = 4 * rows
    assert abs(total - n / 2) <= 6 * np.sqrt(n / 4)                 # binomial(n, 1/2): sigma = sqrt(n) / 2
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(per_call[i], per_call[j])
    assert not np.array_equal(cr.flags(rows, 0.5, 0, SEED + 1), per_call[0])          # the ring's seed is the key
    # the stream is counter word 4: not the draw's (1), the stratified draw's (2) or the mirror's (3)
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for word in (1, 2, 3):
        other = np.array([xo.philox((b, 0, 0, word), key)[0] < 2 ** 31 for b in range(256)], np.uint8)
        assert not np.array_equal(other, per_call[0][:256])
    own = np.array([xo.philox((b, 0, 0, 4), key)[0] < 2 ** 31 for b in range(256)], np.uint8)
    assert np.array_equal(own, per_call[0][:256])
    import mirror_ref as mr
    assert not np.array_equal(mr.flags(rows, 0.5, 0, SEED), per_call[0])
    assert xo.eps_to_u32(1.0) == 2 ** 32 - 1 and xo.eps_to_u32(0.5) == 2 ** 31


def test_stage_leaves_unflagged_rows_alone():
    rng = np.random.default_rng(2)
    fx = dict(S=rng.integers(0, 15, size=(50, 90)).astype(np.uint8), S2=rng.integers(0, 15, size=(50, 90)).astype(np.uint8),
              A=rng.integers(-1, 96, size=50).astype(np.int32))
    side = rng.integers(0, 2, size=50).astype(np.uint8)
    slots = rng.integers(0, 50, size=300)
    st = cr.stage(fx, slots, 0.5, 3, SEED, side=side)
    f = st["flags"].astype(bool)
    assert f.any() and (~f).any() and np.array_equal(st["slot"], slots)
    assert np.array_equal(st["boards"][~f], fx["S"][slots][~f]) and np.array_equal(st["action"][~f], fx["A"][slots][~f])
    assert np.array_equal(st["next_boards"][~f], fx["S2"][slots][~f]) and np.array_equal(st["next_player"][~f], side[slots][~f])
    assert np.array_equal(st["boards"][f], cr.swap_board(fx["S"][slots][f]))
    assert np.array_equal(st["next_boards"][f], cr.swap_board(fx["S2"][slots][f]))
    assert np.array_equal(st["action"][f], cr.swap_action(fx["A"][slots][f]))
    assert np.array_equal(st["next_player"][f], 1 - side[slots][f])
    assert "next_player" not in cr.stage(fx, slots, 0.5, 3, SEED)


# ---- the symmetry itself, on the oracle ---------------------------------------------------------------------------------------------
def swap_code(code):
    f, t = divmod(int(code), 90)
    return int(cr.swap_action(f)) * 90 + int(cr.swap_action(t))


def legal_sets_disagree(boards, image, code_map):
    """every board's list for each colour against the other colour's list on image(board), as sets through code_map
    -> (lists compared, lists that differ, truncated lists, lists that keep their order)"""
    compared = differ = truncated = ordered = 0
    for b in boards:
        ob, om = xo.board_from(b), xo.board_from(image(b))
        for colour in (0, 1):
            codes, n = xo.all_valid_actions(ob, colour)
            mcodes, mn = xo.all_valid_actions(om, 1 - colour)
            compared += 1
            truncated += (n > xo.MAX_MOVES) or (mn > xo.MAX_MOVES)
            mapped = [code_map(c) for c in codes]
            if n != mn or sorted(mapped) != sorted(int(c) for c in mcodes):
                differ += 1
            elif mapped == [int(c) for c in mcodes]:
                ordered += 1
    return compared, differ, truncated, ordered


@pytest.fixture(scope="module")
def sparse(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_sparse.npz"))["board"].astype(np.uint8)


def test_swapped_legal_sets_match_the_other_colours(sparse):
    compared, differ, truncated, ordered = legal_sets_disagree(sparse, cr.swap_board, swap_code)
    print("lists that keep their order under the map: %d of %d" % (ordered, compared))
    assert compared == 1460 and differ == 0 and truncated == 0
    assert ordered < compared                     # the canonical scan order is not symmetric: only sets can be compared


def test_each_half_of_the_map_alone_breaks_the_symmetry(sparse):
    """negative controls: row -> 9 - row without the code map, and the code map without the row exchange, must each fail somewhere"""
    assert np.array_equal(cr.flip_rows(cr.flip_rows(sparse)), sparse) and np.array_equal(cr.swap_codes(cr.swap_codes(sparse)), sparse)
    _, differ, _, _ = legal_sets_disagree(sparse[::5], cr.flip_rows, swap_code)
    assert differ > 0
    _, differ, _, _ = legal_sets_disagree(sparse[::5], cr.swap_codes, int)
    assert differ > 0


def test_move_reward_and_game_over_commute_with_the_colour_swap(sparse):
    L = xo.lib()
    moves = 0
    for b in sparse:
        for colour in (0, 1):
            codes, n = xo.all_valid_actions(xo.board_from(b, player=colour), colour)
            for code in codes:
                f, t = divmod(int(code), 90)
                fm, tm = int(cr.swap_action(f)), int(cr.swap_action(t))
                p, q = xo.board_from(b, player=colour), xo.board_from(cr.swap_board(b), player=1 - colour)
                cap_p = L.xqo_move_piece(C.byref(p), f // 9, f % 9, t // 9, t % 9)
                cap_q = L.xqo_move_piece(C.byref(q), fm // 9, fm % 9, tm // 9, tm % 9)
                assert 0 <= cap_p <= 14 and cap_q == int(cr.SIGMA[cap_p])
                assert np.array_equal(cr.swap_board(p.squares()), q.squares())
                assert p.moveCount == q.moveCount and q.currentPlayer == 1 - p.currentPlayer
                assert (p.redScore, p.blackScore) == (q.blackScore, q.redScore)
                for side in (0, 1):
                    for mc in (p.moveCount, 199, 200):
                        assert L.xqo_evaluate_board(C.byref(p), side, mc) == L.xqo_evaluate_board(C.byref(q), 1 - side, mc)
                assert L.xqo_check_game_over(C.byref(p)) == L.xqo_check_game_over(C.byref(q))
                moves += 1
    assert moves == 30157


# ---- the entry points ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_colour_swap_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_COLOUR_SWAP, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_COLOUR_SWAP) == set(NEW_SYMBOLS)
    assert not set(capi.LAZY_COLOUR_SWAP) & set(capi.LAZY_MIRROR)


def test_colour_swap_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    p, c = C.c_double(), C.c_uint64()
    calls = [("xq_replay_set_colour_swap", (None, 0.5)), ("xq_replay_get_colour_swap", (None, C.byref(p), C.byref(c))),
             ("xq_dqn_last_colour_swap", (None, 1, None, None, None, None, None, None)), ("xq_trainer_set_colour_swap", (None, 0.5))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name


def test_work_model_knows_the_colour_swap_bracket_only_when_asked():
    import cn_chess_ai_amd.workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    base, same, on = wm.step_work(*cfg), wm.step_work(*cfg, colour_swap=False), wm.step_work(*cfg, colour_swap=True)
    assert base == same and "colour_swap_stage" not in base and "per_writeback" not in base
    assert set(on) - set(base) == {"colour_swap_stage"} and all(on[k] == base[k] for k in base)
    assert on["colour_swap_stage"]["hbm_bytes"] == 8192 * 215 and on["colour_swap_stage"]["bound"] == "hbm"
    assert on["colour_swap_stage"]["hbm_bytes"] == wm.step_work(*cfg, mirror=True)["mirror_stage"]["hbm_bytes"]
    # behind the n-step assembly and / or the mirror: in place, and every other bracket as without it
    for other in (dict(n_step=3), dict(mirror=True), dict(n_step=3, mirror=True)):
        off, both = wm.step_work(*cfg, **other), wm.step_work(*cfg, colour_swap=True, **other)
        assert set(both) - set(off) == {"colour_swap_stage"} and all(both[k] == off[k] for k in off), other
        assert both["colour_swap_stage"]["hbm_bytes"] == 8192 * 201
    per = wm.step_work(*cfg, prioritized=True, colour_swap=True)
    assert set(per) - set(wm.step_work(*cfg, prioritized=True)) == {"colour_swap_stage", "per_writeback"}
    perm = wm.step_work(*cfg, prioritized=True, mirror=True, colour_swap=True)
    assert perm["per_writeback"] == wm.step_work(*cfg, prioritized=True, mirror=True)["per_writeback"]
    # under the legal bootstrap the side byte rides along and legal_side_stage is not launched
    legal = wm.step_work(*cfg, bootstrap="legal", colour_swap=True)
    assert set(legal) - set(wm.step_work(*cfg, bootstrap="legal")) == {"colour_swap_stage"}
    assert legal["colour_swap_stage"]["hbm_bytes"] == 8192 * 217
    lm, lm_on = wm.step_work(*cfg, bootstrap="legal", mirror=True), wm.step_work(*cfg, bootstrap="legal", mirror=True, colour_swap=True)
    assert "legal_side_stage" in lm and "legal_side_stage" not in lm_on and lm_on["colour_swap_stage"]["hbm_bytes"] == 8192 * 207
    assert wm.rocprof_kernel("colour_swap_stage", *cfg[:2]) == "colour_swap_stage_kernel("


def build_colour_swap_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "colour_swap_facade.cpp"), os.path.join(BUILD, "colour_swap_facade"))


def test_colour_swap_facade_probe_compiles(capi):
    """xq::ReplayBuffer::setColourSwap / colourSwap, xq::ChessAI::setColourSwap / colourSwap and TrainStats::colour_swap with plain g++
    (no HIP headers)"""
    assert os.path.exists(build_colour_swap_facade_probe())
