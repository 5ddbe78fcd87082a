"""The library's one arg-max rule, as a plain loop: THE FIRST MAXIMUM WINS, A NaN NEVER WINS, AND WHEN NOTHING WINS THE ANSWER IS
ENTRY 0 (dqn.cpp:39-51: maxQ = -inf, bestAction = validActions[0], `q > maxQ` moves both).  Test infrastructure only.

Nothing here is imported from the library or the oracle, and nothing here calls np.argmax (it takes a NaN for the maximum): the greedy
move pick of the env kernel, the oracle's restatements of it and the Double-DQN action are all compared with this loop.
"""
import numpy as np


def first_max(values):
    """index of the first strict maximum of `values`; 0 when no value exceeds -inf (all NaN, all -inf, empty)"""
    best, idx = float("-inf"), 0
    for k, v in enumerate(values):
        v = float(v)                 # exact for every float32, denormals and signed zeros included
        if v > best:                 # False for a NaN, for -inf against -inf and for -0.0 against +0.0
            best, idx = v, k
    return idx


def pick(q_row_f32, codes):
    """the greedy move: first_max over q[code % 90] along a move list -> index into the list"""
    q = np.asarray(q_row_f32, dtype=np.float32)
    return first_max(q[int(c) % 90] for c in codes)
