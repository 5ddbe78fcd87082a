"""Reference of the colour-swap augmentation (include/xq_capi.h, xq_replay_set_colour_swap; DESIGN.md §4 "Colour-swap augmentation"):
plain numpy over xqoracle.philox.  The image of a 90-byte board under the exchange of the colours with row -> 9 - row, the action rule,
the flag rule, and stage(): the batch a colour-swap-mode TD step stages.  No device, no library: the GPU tests compare the library with
stage()."""
import numpy as np

import xqoracle as xo

SIGMA = np.array([0, 8, 9, 10, 11, 12, 13, 14, 1, 2, 3, 4, 5, 6, 7, 15], np.uint8)     # 0 stays, 1..7 + 7, 8..14 - 7 (15: no piece code)
ROWS = 9 - np.arange(10)


def swap_codes(boards):
    """the code map alone, squares in place (alone it is a WRONG symmetry: negative control)"""
    return SIGMA[np.asarray(boards, np.uint8)]


def flip_rows(boards):
    """row -> 9 - row alone, codes as they are (alone it is a WRONG symmetry: negative control); [..., 96] nibble arrays keep their last six"""
    b = np.asarray(boards)
    out = b.copy()
    sq = b[..., :90].reshape(b.shape[:-1] + (10, 9))
    out[..., :90] = sq[..., ROWS, :].reshape(b.shape[:-1] + (90,))
    return out


def swap_board(boards):
    """board'[(9 - r) 9 + c] = sigma(board[r 9 + c]) of [..., 90] piece codes (row-major 10 x 9); [..., 96] nibble arrays keep their
    last six entries (which are 0)"""
    return flip_rows(swap_codes(boards))


def pack(board90):
    """the twelve words of a packed board: square s is nibble s & 7 of word s >> 3; nibbles 90..95 are 0"""
    nib = np.zeros(96, np.uint64)
    nib[:90] = np.asarray(board90, np.uint64) & 15
    return [int(sum(int(nib[8 * w + k]) << (4 * k) for k in range(8))) for w in range(12)]


def swap_action(a):
    """a' = a + 81 - 18 (a div 9) for a square 0..89; anything else (-1: dead or empty, 90..95, ...) as it is"""
    a = np.asarray(a, np.int64)
    inside = (a >= 0) & (a < 90)
    return np.where(inside, a + 81 - 18 * (np.where(inside, a, 0) // 9), a).astype(np.int32)


def flags(rows, prob, call, seed):
    """flag_b = (prob == 1) || philox4x32_10({b, 0, call, 4}, seed).v[0] < floor(prob 2^32), saturated"""
    if prob == 1:
        return np.ones(rows, np.uint8)
    thresh = xo.eps_to_u32(prob)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.array([xo.philox((b, 0, call & 0xFFFFFFFF, 4), key)[0] < thresh for b in range(rows)], dtype=np.uint8)


def apply(S, A, S2, side, prob, call, seed):
    """the flagged rows of a batch (boards S, actions A, next boards S2, side to move in s' or None) with their colours exchanged
    -> dict(flags, boards, next_boards, action[, next_player])"""
    S, S2, A = np.asarray(S, np.uint8), np.asarray(S2, np.uint8), np.asarray(A, np.int32)
    f = flags(len(A), prob, call, seed)
    m = f.astype(bool)
    out = dict(flags=f, boards=np.where(m[:, None], swap_board(S), S), next_boards=np.where(m[:, None], swap_board(S2), S2),
               action=np.where(m, swap_action(A), A).astype(np.int32))
    if side is not None:
        side = np.asarray(side, np.uint8)
        out["next_player"] = np.where(m, 1 - side, side).astype(np.uint8)
    return out


def stage(fx, slots, prob, call, seed, side=None):
    """The batch a colour-swap-mode TD step with n_step == 1 and no mirror stages from ring contents fx (S, A, S2 by slot) for the
    sampled `slots`, as DQN.last_colour_swap reports it; side: the ring's side column by slot (legal-move bootstrap) or None.  Reward
    and done are the slots' own."""
    slots = np.asarray(slots, np.int32)
    out = apply(fx["S"][slots], fx["A"][slots], fx["S2"][slots], None if side is None else np.asarray(side)[slots], prob, call, seed)
    out["slot"] = slots
    return out
