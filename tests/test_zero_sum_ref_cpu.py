"""CPU checks of the zero-sum TD target's definition (tests/zero_sum_ref.py; DESIGN.md §4 "Zero-sum target"), not gpu:

1. the written-out rule equals batch_ref / nstep_ref called with -gamma (1e-12 in fp64, bit for bit in the fp32 chain), n = 1..8;
2. negative controls: the `+` rule and the same-sign n-step sum are told apart on every row that can show it;
3. a known answer: on a hand-written game tree the zero-sum target iterates to the negamax values, the `+` target to others;
4. the legal-move bootstrap: a side without a piece (tests/sparse_boards.py) is worth -1, y = r + gamma, every other row untouched.
"""
import numpy as np
import pytest

import batch_ref as br
import legal_ref as lr
import nstep_ref as nr
import sparse_boards as sb
import xqoracle as xo
import zero_sum_ref as zr

SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.97


def _params(sizes, seed):
    w, _ = xo.init_weights(sizes, seed)
    b = np.random.default_rng(seed + 100).uniform(-0.05, 0.05, size=xo.nn_counts(sizes)[1])
    return w * 4.0, b


def _batch(n, seed):
    """n transitions on legal-to-push boards with done rows, dead rows (action -1) and rewards of both signs"""
    rng = np.random.default_rng(seed)
    S, S2 = nr.random_boards(rng, n), nr.random_boards(rng, n)
    A = rng.integers(0, 90, n).astype(np.int32)
    A[rng.random(n) < 0.1] = -1
    D = (rng.random(n) < 0.2).astype(np.uint8)
    A[:3], D[:3] = [5, -1, 9], [1, 0, 0]
    R = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    return S, A, R, D, S2


def _close(got, want, what):
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(got - want).max() <= 1e-12 * scale, (what, float(np.abs(got - want).max() / scale))


# ---- 1. the written-out rule is the existing references at -gamma ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_written_out_rule_equals_batch_ref_at_minus_gamma(rule, prec):
    n = 40
    S, A, R, D, S2 = _batch(n, seed=3)
    assert D.any() and not D.all() and (A < 0).any()
    w, b = _params(SMALL_NET, 5)
    wt, bt = _params(SMALL_NET, 6)
    net, tnet = br.Net(SMALL_NET, w, b, prec), br.Net(SMALL_NET, wt, bt, prec)
    f = zr.forward(net, S, S2, A, R, D, GAMMA, rule, prec, target_net=tnet)
    g = br.forward(net, S, S2, A, R, D, -GAMMA, rule, prec, target=tnet)
    _close(f.q, g.q, "q"); _close(f.y, g.y, "y")
    assert np.array_equal(f.astar, g.astar) and np.array_equal(f.live, g.live)
    _close(zr.target(R, D, f.tanh_zm, GAMMA), g.y, "target()")
    if rule == 2:
        for a, c in zip(f.cand_y, g.cand_y):
            assert (a is None) == (c is None)
            if a is not None:
                _close(a, c, "cand_y")
    # ... and so is the whole step: deltas and gradient sums, with importance weights
    wts = np.random.default_rng(1).uniform(0.1, 1.0, n)
    mode = 1
    bk = br.backward(net, f, mode, prec, wts)
    u = br.accumulate(net, f, bk, prec)
    net2, f2, bk2, u2 = br.td_step(SMALL_NET, w, b, S, S2, A, R, D, -GAMMA, rule, mode, prec, wts, wt, bt)
    _close(bk.dout, bk2.dout, "dout")
    for l in range(net.nl):
        _close(u.gW[l], u2.gW[l], ("gW", l)); _close(u.gB[l], u2.gB[l], ("gB", l))


@pytest.mark.parametrize("n", list(range(1, 9)))
def test_alternating_discounts_and_returns_equal_nstep_ref_at_minus_gamma_bit_for_bit(n):
    d, e = zr.discounts(GAMMA, n), nr.discounts(-GAMMA, n)
    assert len(d) == len(e) == n + 1
    assert np.array_equal(np.array(d, np.float32).view(np.uint32), np.array(e, np.float32).view(np.uint32))
    mags = nr.discounts(GAMMA, n)
    for k in range(n + 1):
        assert d[k] == (mags[k] if k % 2 == 0 else -mags[k]) and d[k].dtype == np.float32
    seen = set()
    for name in nr.FIXTURES:
        fx = nr.named_fixture(name)
        first, count = nr.readable(fx["cap"], fx["size"], fx["write_pos"])
        slots = nr.all_slots(fx)
        got = zr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], GAMMA, first, count)
        want = nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], -GAMMA, first, count)
        assert np.array_equal(got["reward"].view(np.uint32), want["reward"].view(np.uint32))
        for k in ("done", "steps", "first_slot", "last_slot", "action", "dead"):
            assert np.array_equal(got[k], want[k]), k
        assert got["cls"] == want["cls"]
        seen |= set(got["cls"])
    if n >= 3:                                          # done and empty slots inside chains
        assert {"empty_mid", "incomplete", "full", "empty0"} <= seen and any(c.startswith("done") and c != "done1" for c in seen)


# ---- 2. negative controls ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_the_plus_rule_leaves_the_tolerance_on_every_row_that_bootstraps(rule):
    n = 40
    S, A, R, D, S2 = _batch(n, seed=4)
    w, b = _params(SMALL_NET, 5)
    wt, bt = _params(SMALL_NET, 6)
    net, tnet = br.Net(SMALL_NET, w, b), br.Net(SMALL_NET, wt, bt)
    f = zr.forward(net, S, S2, A, R, D, GAMMA, rule, target_net=tnet)
    plus = br.forward(net, S, S2, A, R, D, GAMMA, rule, target=tnet)
    rows = f.live & ~f.D & (f.tanh_zm != 0)
    assert rows.sum() >= n // 2
    yerr = np.abs(plus.y - f.y) / np.maximum(1.0, np.abs(f.y))            # check_q_y's measure
    assert (yerr[rows] >= br.QTOL).all()
    assert f.D.any() and np.array_equal(plus.y[f.D], f.y[f.D])             # done rows: y = r under both (dead rows have no target)
    if rule != 2:
        with pytest.raises(AssertionError):
            br.check_q_y(f, plus.q, plus.y, br.PRECISION_F32)
    br.check_q_y(f, f.q, f.y, br.PRECISION_F32)


@pytest.mark.parametrize("n", list(range(2, 9)))
def test_the_same_sign_n_step_sum_differs_on_every_row_with_a_second_reward(n):
    hit = 0
    for name in nr.FIXTURES:
        fx = nr.named_fixture(name)
        first, count = nr.readable(fx["cap"], fx["size"], fx["write_pos"])
        slots = nr.all_slots(fx)
        got = zr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], GAMMA, first, count)
        same = nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], GAMMA, first, count)
        r1 = fx["R"][(first + (slots - first) % fx["cap"] + fx["stride"]) % fx["cap"]]
        rows = (got["steps"] >= 2) & (r1 != 0)
        hit += int(rows.sum())
        assert (got["reward"][rows] != same["reward"][rows]).all()
        one = got["steps"] == 1
        assert np.array_equal(got["reward"][one], same["reward"][one])
    assert hit >= 20


# ---- 3. a known answer: this is negamax --------------------------------------------------------------------------------------------------
def test_iterating_the_zero_sum_target_gives_the_negamax_values_of_a_small_game():
    """Three positions; the sides alternate, every reward is the mover's own.
         P0 (X to move):  a -> P1, r = 0      b -> P2, r = 0.2   (b takes a pawn and leaves the general hanging)
         P1 (O to move):  c -> end, r = 0.1
         P2 (O to move):  d -> end, r = 0.9  (O takes the general)
    negamax by hand: V(P1) = 0.1, V(P2) = 0.9, Q(P0, a) = 0 - g 0.1, Q(P0, b) = 0.2 - g 0.9, so X plays a and V(P0) = -g 0.1.
    The `+` target gives Q(P0, b) = 0.2 + g 0.9: the blunder is the best move on the board."""
    g = 0.9
    # (state, action) -> (reward, next state or None)
    T = {(0, 0): (0.0, 1), (0, 1): (0.2, 2), (1, 0): (0.1, None), (2, 0): (0.9, None)}
    acts = {0: (0, 1), 1: (0,), 2: (0,)}

    def iterate(sign):
        Q = {k: 0.0 for k in T}
        for _ in range(5):
            Q = {(s, a): r if s2 is None else r + sign * g * max(Q[(s2, a2)] for a2 in acts[s2]) for (s, a), (r, s2) in T.items()}
        return Q

    def negamax(s):
        return max(r if s2 is None else r - g * negamax(s2) for (st, a), (r, s2) in T.items() if st == s)

    Qz, Qp = iterate(-1.0), iterate(+1.0)
    want = {(0, 0): -0.09, (0, 1): 0.2 - 0.81, (1, 0): 0.1, (2, 0): 0.9}
    for k in T:
        assert abs(Qz[k] - want[k]) < 1e-15, k
    for s in acts:
        assert abs(max(Qz[(s, a)] for a in acts[s]) - negamax(s)) < 1e-15
    assert max(acts[0], key=lambda a: Qz[(0, a)]) == 0                    # the zero-sum learner keeps its general
    plus = {(0, 0): 0.09, (0, 1): 0.2 + 0.81, (1, 0): 0.1, (2, 0): 0.9}
    for k in T:
        assert abs(Qp[k] - plus[k]) < 1e-15, k
    assert max(acts[0], key=lambda a: Qp[(0, a)]) == 1                    # the `+` learner hangs it
    assert abs(Qp[(0, 1)] - Qz[(0, 1)]) == pytest.approx(2 * g * 0.9)
    # the same answer from zero_sum_ref.target, one backup at a time (tanh(zm) stands for the table's best next value)
    v1, v2 = zr.target([0.1, 0.9], [1, 1], [0.0, 0.0], g)
    q0 = zr.target([0.0, 0.2], [0, 0], [v1, v2], g)
    assert np.allclose(q0, [want[(0, 0)], want[(0, 1)]], atol=1e-15)


# ---- 4. a side that cannot move has lost -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_rows_whose_side_to_move_has_no_piece_get_r_plus_gamma_and_no_other_row_moves(rule):
    n = 48
    rng = np.random.default_rng(8)
    S = nr.random_boards(rng, n)
    e_boards, e_meta = sb.gen_arbitrary(n // 2, seed=3, empty_mover=True)
    o_boards, o_meta = sb.gen_endgames(n - n // 2, seed=4)
    S2 = np.concatenate([e_boards, o_boards])
    side = np.concatenate([e_meta[:, 1], o_meta[:, 1]]).astype(np.uint8)
    A = rng.integers(0, 90, n).astype(np.int32)
    D = np.zeros(n, np.uint8)
    A[[1, 30]] = -1
    D[[2, 5, 31]] = 1
    R = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    w, b = _params(SMALL_NET, 5)
    wt, bt = _params(SMALL_NET, 6)
    net, tnet = br.Net(SMALL_NET, w, b), br.Net(SMALL_NET, wt, bt)
    f = zr.legal_forward(net, S, S2, A, R, D, side, GAMMA, rule, target_net=tnet)
    plain = lr.forward(net, S, S2, A, R, D, side, GAMMA, rule, target=tnet)
    minus = lr.forward(net, S, S2, A, R, D, side, -GAMMA, rule, target=tnet)
    stuck = f.n_moves == 0
    assert stuck.sum() >= n // 2 - 4 and (f.D & f.live).sum() >= 1 and (f.n_moves > 0).sum() >= 10
    assert np.array_equal(f.n_moves, plain.n_moves) and np.array_equal(f.astar, plain.astar)
    Rd = R.astype(np.float64)
    _close(f.y[stuck], Rd[stuck] + GAMMA, "no move")
    assert np.array_equal(plain.y[stuck], Rd[stuck])                     # today: y = r
    assert np.isneginf(f.zmax[stuck]).all() and (plain.zmax[stuck] == 0).all()
    # every other row is legal_ref at -gamma, which knows nothing of the no-move value
    _close(f.y[~stuck], minus.y[~stuck], "other rows")
    assert np.array_equal(minus.y[stuck], Rd[stuck])
    done = f.D | ~f.live
    assert np.array_equal(f.y[done], Rd[done])
    moved = f.n_moves > 0
    ze = lr.z96(net if rule == 0 else tnet, S2)
    _close(f.y[moved], Rd[moved] - GAMMA * np.tanh(ze[moved, f.astar[moved]]), "rows with a move")
    assert np.array_equal(f.zmax[~stuck], plain.zmax[~stuck])
