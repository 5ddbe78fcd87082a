"""Reference of the mover view (include/xq_capi.h, xq_dqn_set_view; DESIGN.md §4 "Mover view"): plain numpy on top of
tests/colour_swap_ref.py.  view(board, side) is the board for Red (side 0) and its colour swap for Black (side 1); a transition
(s, a, r, s', done) with mover m and next side p trains on (view(s, m), m ? swap(a) : a, r, view(s', p), done), and in that batch the side
to move in s' is always Red.  No device, no library: the GPU tests compare the library with stage()."""
import numpy as np

import colour_swap_ref as cr


def view(boards, side):
    """view(board, side) of [n, 90] piece codes ([n, 96] nibble arrays keep their last six) and [n] sides: side 0 -> the board, anything
    else -> swap(board)"""
    b = np.asarray(boards, np.uint8)
    m = np.asarray(side).reshape(-1) != 0
    return np.where(m[:, None], cr.swap_board(b), b)


def view_action(a, side):
    """the action as the net with the view indexes it: swap(a) where Black moved"""
    a = np.asarray(a, np.int32)
    return np.where(np.asarray(side).reshape(-1) != 0, cr.swap_action(a), a).astype(np.int32)


def apply(S, A, S2, mover, next_player):
    """a batch (boards S, actions A, next boards S2) with who moved in s and who moves in s' per row
    -> dict(flag_s, flag_next, boards, next_boards, action, next_player): next_player is what a legal-bootstrap step is given, 0 on
    every row"""
    m = (np.asarray(mover).reshape(-1) != 0).astype(np.uint8)
    p = (np.asarray(next_player).reshape(-1) != 0).astype(np.uint8)
    return dict(flag_s=m, flag_next=p, boards=view(S, m), next_boards=view(S2, p), action=view_action(A, m),
                next_player=np.zeros(len(m), np.uint8))


def stage(fx, slots, mover, next_player):
    """The batch a view-mode TD step with n_step == 1 and no mirror stages from ring contents fx (S, A, S2 by slot) for the sampled
    `slots`, as DQN.last_view reports it; mover / next_player: the ring's two side columns by slot.  Reward and done are the slots'
    own."""
    slots = np.asarray(slots, np.int32)
    out = apply(fx["S"][slots], fx["A"][slots], fx["S2"][slots], np.asarray(mover)[slots], np.asarray(next_player)[slots])
    out["slot"] = slots
    return out


def pick_rows(q, side):
    """Q rows [n, 90] indexed by absolute destination -> the rows a view net would have to put out for the same values: for Black games
    row'[swap(t)] = row[t], for Red games the row"""
    q = np.asarray(q)
    perm = cr.swap_action(np.arange(90))
    out = q.copy()
    black = np.flatnonzero(np.asarray(side).reshape(-1) != 0)
    out[np.ix_(black, perm)] = q[black][:, :90]
    return out
