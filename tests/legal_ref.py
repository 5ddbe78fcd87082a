"""fp64 restatement of the legal-move TD bootstrap (xq_dqn_set_td_bootstrap, DESIGN.md §4 "Legal-move bootstrap").  Test infrastructure
only, like batch_ref.py: tests import it, the product path never does.

    y = done ? r : r + gamma * tanh(z_eval(s')[to*]),   to* = to_k of the first maximum of z_sel(s')[to_k] over the move list

(from_k, to_k) runs over getAllValidActions(s', side) in the canonical order — the oracle's rules engine — cut to its first 128
entries; z is the output layer's pre-activation.  z_sel and z_eval are the online net's for td_rule 0, the target net's for 1, and the
online / the target net's for 2 (Double DQN).  A NaN never wins, nothing wins: entry 0; an empty list: y = r.

The winner is found here with numpy on masked values; tests/test_legal_ref_cpu.py holds it to the loop of tests/first_max.py.
"""
import numpy as np

import batch_ref as br
import xqoracle as xo

MAX_MOVES = 128


def move_list(board90, side):
    """codes (from * 90 + to, uint16) of getAllValidActions(board, side) in the canonical order, at most MAX_MOVES of them"""
    codes, n = xo.all_valid_actions(xo.board_from(np.asarray(board90, dtype=np.uint8), player=int(side)), int(side))
    return np.asarray(codes[:min(int(n), MAX_MOVES)], dtype=np.uint16)


_rows = {}


def fixture_rows(golden_dir, name):
    """(boards [2 N][90], sides [2 N], lists) of a rules fixture (ref_bigmoves.npz, ref_sparse.npz): every board once with Red and once
    with Black to move (rows 2 i and 2 i + 1), the lists the REAL reference engine's `red` / `black` records cut to MAX_MOVES."""
    import os
    if name not in _rows:
        t = np.load(os.path.join(golden_dir, name))
        boards = np.repeat(t["board"].astype(np.uint8), 2, axis=0)
        sides = np.tile(np.array([0, 1], np.uint8), len(t["board"]))
        lists = []
        for i in range(len(t["board"])):
            for key in ("red", "black"):
                lists.append(np.asarray(t[key][t[key + "_off"][i]:t[key + "_off"][i + 1]][:MAX_MOVES], dtype=np.uint16))
        _rows[name] = (boards, sides, lists)
    return _rows[name]


def select(values):
    """index of the winner among `values` (z[to_k] in list order): the first maximum, a NaN never wins, nothing above -inf: 0"""
    v = np.asarray(values, dtype=np.float64)
    if len(v) == 0:
        return 0
    v = np.where(np.isnan(v), -np.inf, v)
    m = v.max()
    return 0 if m == -np.inf else int(np.flatnonzero(v == m)[0])


def pick_rows(z, lists):
    """per row of z [n][>= 90] (any float type, compared as given) and its move list: (a_star: the winning `to`, -1 for an empty list;
    zmax: z[a_star] in z's dtype, 0 for an empty list)"""
    z = np.asarray(z)
    a = np.full(len(lists), -1, np.int32)
    zm = np.zeros(len(lists), z.dtype)
    for i, codes in enumerate(lists):
        if len(codes) == 0:
            continue
        tos = np.asarray(codes, dtype=np.int64) % 90
        a[i] = tos[select(z[i, tos])]
        zm[i] = z[i, a[i]]
    return a, zm


def z96(net, next_boards, chunk=br.CHUNK):
    """fp64 pre-activations of outputs 0..95 of every next board on `net` (a batch_ref.Net)"""
    x = br._inputs(next_boards)
    z = np.empty((len(x), 96))
    for c0 in range(0, len(x), chunk):
        a_last = net.hidden(br.one_hot(x[c0:c0 + chunk]))[-1]
        z[c0:c0 + chunk] = net.Bf[-1][:96] + a_last @ net.Wf[-1][:96].T
    return z


def forward(net, boards, next_boards, A, R, D, side, gamma, td_rule=0, target=None, precision=br.PRECISION_F32, lists=None):
    """batch_ref.forward under the legal-move bootstrap: a batch_ref.Forward (q, y, astar, acts, cand_y ... as backward / accumulate /
    check_q_y / check_update take them) with, per row, n_moves (-1 on done rows and dead ones, action < 0), astar (the winning `to`,
    -1 without one), zmax (the selecting net's z of it), z96 (the selecting net's rows), cands (the `to` within CAND_MARGIN of the
    maximum) and, for every rule, cand_y (the y of each candidate).  lists: the rows' move lists if the caller has them."""
    n = len(br._inputs(boards))
    D = np.asarray(D).reshape(n).astype(bool)
    side = np.asarray(side).reshape(n)
    f = br.forward(net, boards, next_boards, A, R, np.ones(n, bool), gamma, 0, precision)      # Q(s,a) and the activations; y = r
    f.D, f.td_rule = D, td_rule
    sel = target if td_rule == 1 else net
    ev = net if td_rule == 0 else target
    assert sel is not None and ev is not None
    zs = z96(sel, next_boards)
    ze = zs if ev is sel else z96(ev, next_boards)
    margin = br.CAND_MARGIN[precision]
    f.z96, f.n_moves, f.zmax = zs, np.full(n, -1, np.int32), np.zeros(n)
    f.cands = [None] * n
    nb = br._inputs(next_boards)
    for i in range(n):
        if D[i] or not f.live[i]:
            continue
        codes = move_list(nb[i], side[i]) if lists is None else lists[i]
        f.n_moves[i] = len(codes)
        if len(codes) == 0:
            continue
        tos = np.asarray(codes, dtype=np.int64) % 90
        to = int(tos[select(zs[i, tos])])
        f.astar[i], f.zmax[i] = to, zs[i, to]
        f.y[i] = f.R[i] + gamma * np.tanh(ze[i, to])
        cand = np.unique(tos[zs[i, tos] >= zs[i, to] - margin])
        f.cands[i] = cand
        f.cand_y[i] = f.R[i] + gamma * np.tanh(ze[i, cand])
    return f


def all_outputs_y(net, next_boards, R, D, gamma):
    """the default rule's y on the same rows: r + gamma * tanh(max over ALL outputs of z(s'))"""
    x = br._inputs(next_boards)
    z = net.z_out(net.hidden(br.one_hot(x))[-1])
    R = np.asarray(R, dtype=np.float64)
    return np.where(np.asarray(D).astype(bool), R, R + gamma * np.tanh(z.max(axis=1)))
