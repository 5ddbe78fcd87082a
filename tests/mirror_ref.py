"""Reference of the mirror augmentation (include/xq_capi.h, xq_replay_set_mirror; DESIGN.md §4 "Mirror augmentation"): plain numpy over
xqoracle.philox.  The reflection of a 90-byte board, the action rule, the flag rule, and stage(): the batch a mirror-mode TD step stages.
No device, no library: the GPU tests compare the library with stage()."""
import numpy as np

import xqoracle as xo

COLS = 8 - np.arange(9)


def reflect(boards):
    """col -> 8 - col of [..., 90] piece codes (row-major 10 x 9); [..., 96] nibble arrays keep their last six entries (which are 0)"""
    b = np.asarray(boards)
    out = b.copy()
    sq = b[..., :90].reshape(b.shape[:-1] + (10, 9))
    out[..., :90] = sq[..., COLS].reshape(b.shape[:-1] + (90,))
    return out


def reflect_rows(boards):
    """the WRONG reflection (negative control): row -> 9 - row"""
    b = np.asarray(boards)
    return b.reshape(b.shape[:-1] + (10, 9))[..., ::-1, :].reshape(b.shape)


def pack(board90):
    """the twelve words of a packed board: square s is nibble s & 7 of word s >> 3; nibbles 90..95 are 0"""
    nib = np.zeros(96, np.uint64)
    nib[:90] = np.asarray(board90, np.uint64) & 15
    return [int(sum(int(nib[8 * w + k]) << (4 * k) for k in range(8))) for w in range(12)]


def mirror_action(a):
    """a' = a - 2 (a mod 9) + 8 for a square 0..89; anything else (-1: dead or empty, 90..95, ...) as it is"""
    a = np.asarray(a, np.int64)
    inside = (a >= 0) & (a < 90)
    return np.where(inside, a - 2 * (np.where(inside, a, 0) % 9) + 8, a).astype(np.int32)


def flags(rows, prob, call, seed):
    """flag_b = (prob == 1) || philox4x32_10({b, 0, call, 3}, seed).v[0] < floor(prob 2^32), saturated"""
    if prob == 1:
        return np.ones(rows, np.uint8)
    thresh = xo.eps_to_u32(prob)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.array([xo.philox((b, 0, call & 0xFFFFFFFF, 3), key)[0] < thresh for b in range(rows)], dtype=np.uint8)


def apply(S, A, S2, prob, call, seed):
    """the flagged rows of a batch (boards S, actions A, next boards S2) reflected -> dict(flags, boards, next_boards, action)"""
    S, S2, A = np.asarray(S, np.uint8), np.asarray(S2, np.uint8), np.asarray(A, np.int32)
    f = flags(len(A), prob, call, seed)
    m = f.astype(bool)
    return dict(flags=f, boards=np.where(m[:, None], reflect(S), S), next_boards=np.where(m[:, None], reflect(S2), S2),
                action=np.where(m, mirror_action(A), A).astype(np.int32))


def stage(fx, slots, prob, call, seed):
    """The batch a mirror-mode TD step with n_step == 1 stages from ring contents fx (S, A, S2 by slot) for the sampled `slots`, as
    DQN.last_mirror reports it.  Reward and done are the slots' own."""
    slots = np.asarray(slots, np.int32)
    out = apply(fx["S"][slots], fx["A"][slots], fx["S2"][slots], prob, call, seed)
    out["slot"] = slots
    return out
