"""The Boltzmann pick of the env kernel (xq_env_set_policy, DESIGN.md §4 "Exploration policy"), as its definition in fp64 numpy.  Test
infrastructure only: nothing here is imported from the library or the oracle.

For the legal list in its canonical order, i = 0 .. n-1, n <= 128, on a ply that did not take the epsilon branch and reads Q rows:

  v_i     the value the greedy pick compares: q[to_i], q[swap(to_i)] for Black under the q-view; a NaN counts as -inf
  m       max v_i.  Not finite (every candidate -inf or NaN, or a +inf present): the pick is the first maximum (tests/first_max.py)
  x_i     fl32(fl32(v_i - m) * it), it = (float)(1.0 / T) formed in double: a difference and a product, rounded to fp32 once each
  w_i     exp(x_i), 0 where v_i = -inf and where fp32's expf underflows to an exact zero (x_i < -104; ln 2^-150 = -103.97)
  u       (r2 >> 8) * 2^-24, r2 = word 2 of the ply's Philox block (word 0: epsilon, word 1: the uniform index)
  t       u * sum w
  pick    the first i whose inclusive prefix sum exceeds t; the last i with w_i > 0 if none does

The device forms w_i with its own expf and sums in another order, so a draw that falls on a boundary may resolve either way.  Each w_i
carries at most w_i (|x_i| + 4) 2^-23 of error (two roundings of x, expf within a few ulp), the scan adds at most 8 levels and t one
rounding: a draw is UNDECIDED when |t - C_j| <= beta * total for a prefix sum C_j, beta = 2^-22 (max{|x_i| : w_i > 0} + 4) + 2^-20.
"""
import numpy as np

F32 = np.float32
NEG = float("-inf")
X_ZERO = -104.0                 # below it expf(x) is an exact fp32 zero
MAX_UNDECIDED = 0.02            # at most this share of the draws of one test case may be undecided


def inv_temperature(T):
    return F32(1.0 / float(T))


def swap_square(t):
    """the colour swap's square map: row -> 9 - row"""
    return t + 81 - 18 * (t // 9)


def values(q_row, codes, swap=False):
    """v_i as float32: q[to_i] (q[swap(to_i)] with swap), NaN -> -inf"""
    to = np.asarray(codes, dtype=np.int64) % 90
    if swap:
        to = swap_square(to)
    v = np.asarray(q_row, dtype=F32)[to].copy()
    v[np.isnan(v)] = NEG
    return v


def first_max(v):
    """index of the first strict maximum; 0 when nothing exceeds -inf (a plain loop: np.argmax takes a NaN for the maximum)"""
    best, idx = NEG, 0
    for k, x in enumerate(v):
        x = float(x)
        if x > best:
            best, idx = x, k
    return idx


def weights(v, T):
    """(w [n] float64, x [n] float32) of a candidate vector with a finite maximum"""
    v = np.asarray(v, dtype=F32)
    m = v.max()
    with np.errstate(invalid="ignore"):
        d = (v - m).astype(F32)                                       # one rounding
        x = (d * inv_temperature(T)).astype(F32)                     # ... and another
    w = np.where((v == NEG) | (x < X_ZERO), 0.0, np.exp(x.astype(np.float64)))
    return w, x


def beta(w, x):
    return 2.0 ** -22 * (float(np.abs(x[w > 0]).max()) + 4.0) + 2.0 ** -20


def pick_many(v, T, r2):
    """the picks of one candidate vector for an array of Philox words r2 -> (idx [k] int64, undecided [k] bool).  idx is the first
    maximum for every draw when the maximum is not finite; never undecided then."""
    v = np.asarray(v, dtype=F32)
    r2 = np.atleast_1d(np.asarray(r2, dtype=np.uint64))
    m = float(v.max()) if len(v) else NEG
    if not np.isfinite(m):
        return np.full(len(r2), first_max(v), np.int64), np.zeros(len(r2), bool)
    w, x = weights(v, T)
    C = np.cumsum(w)                                                  # fp64, left to right
    total = C[-1]
    u = (r2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    t = u * total
    idx = np.searchsorted(C, t, side="right")                         # the first i with C_i > t
    last = int(np.nonzero(w > 0)[0][-1])
    idx = np.where(idx >= len(C), last, idx).astype(np.int64)
    # the nearest prefix sum on either side of t
    k = np.clip(np.searchsorted(C, t, side="left"), 0, len(C) - 1)
    near = np.minimum(np.abs(C[k] - t), np.abs(C[np.maximum(k - 1, 0)] - t))
    return idx, near <= beta(w, x) * total


def pick(v, T, r2):
    """-> (index into the list, undecided)"""
    idx, und = pick_many(v, T, [r2])
    return int(idx[0]), bool(und[0])


def step(q_row, codes, T, r, eps_u32=0, swap=False):
    """One ply's pick by the whole rule.  r: the four Philox words of the ply; T: None or 0 = greedy.
    -> (index into the list, `explored` as xq_step_result reports it: 1 epsilon branch, 2 a Boltzmann draw left the first maximum,
    else 0, undecided)"""
    n = len(codes)
    if int(r[0]) < int(eps_u32):
        return int(r[1]) % n, 1, False
    v = values(q_row, codes, swap)
    fm = first_max(v)
    if not T:
        return fm, 0, False
    idx, und = pick(v, T, int(r[2]))
    return idx, (2 if idx != fm else 0), und


def softmax(v, T):
    """the analytic distribution the draws follow, in fp64 on the fp32 x_i of the rule"""
    w, _ = weights(v, T)
    return w / w.sum()
