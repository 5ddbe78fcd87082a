"""The table of priority tables and draws that sit on the capacity-dependent paths of the prioritized-replay kernels (csrc/xq_replay.hip),
shared by tests/test_per_ref_cpu.py (the oracle against the fp64 reference of tests/per_ref.py) and tests/test_per_shape_edges_gpu.py (the
device against both).  Test infrastructure only.

Capacities: one on each side of every change of the tree's shape (nodes per level, leaves first):
    1                   [1]                  no level kernel at all; the root is leaf 0
    2, 31, 32           [cap, 1]             per_upper_kernel's level loop runs zero times; one descent step
    33, 1024            3 levels             first use of that loop
    1025, 5000, 32768   4 levels
    32769, 1048576      5 levels             the workload's shape (1 M slots)
    1048577             6 levels, n[2] = 1025 > 1024 threads: the stride of the level loop runs
    2097153             6 levels, n[1] = 65537: 1028 wave counts > 1024 threads: the stride of the count sum runs
Batches 1, 63, 64, 65, 1000, 16384: partial waves and partial blocks of per_sample_kernel, and the workload's batch.  All six at 33, 32769
and 1048577 (two cases of three draws); a pair at every other capacity, always with one batch of 1000 or more — far more than the
eligible slots of the small rings and of `one`, so duplicates are certain.

The top of the mass range.  The last stratum's u = fl(fl(B - 1 + r) * fl(total / B)) reaches the fp32 total itself when B - 1 + r rounds up
to B: at B = 16384 for r > 1 - 2^-11, one draw in 2048.  That mass falls off the end of the root's children, the one place where the
descent's fall-off rule decides a slot by itself; random seeds almost never show it.  TOP_SEED is a ring seed whose call 0 has such an r
(`reaches_top`, asserted by the CPU test); the `top` cases draw with it over tables whose last slots are positive (`uni`) and zero
(`endzeros`), at capacities with a full last node per level (1024, 32768, 1048576) and with a nearly empty one (33, 5000, 32769, 1048577).
"""
import functools
from collections import namedtuple

import numpy as np

CAPACITIES = (1, 2, 31, 32, 33, 1024, 1025, 5000, 32768, 32769, 1048576, 1048577, 2097153)
FULL_BATCH_SET = (33, 32769, 1048577)         # also the capacities of the retire-window test
BATCHES = (1, 63, 64, 65, 1000, 16384)
_TRIPLES = ((1, 64, 16384), (63, 65, 1000))
_PAIRS = ((1, 16384), (63, 1000), (64, 16384), (65, 1000))
TABLES = ("uni", "wide", "heavy", "endzeros", "one", "empty")

P_FLOOR = np.float32(1e-3 ** 0.6)     # (|e| + eps)^alpha at e = 0 with the workload's eps = 1e-3, alpha = 0.6
P_HEAVY = np.float32(2.0 ** 0.6)      # ... and at the largest TD error of tanh outputs, |e| = 2

TOP_SEED = 0xFEFA63                   # philox([16383, 0, 0, 2], TOP_SEED)[0] >> 8 = 0xFFF8BF: 16383 + r rounds to 16384.0f
TOP_CAPACITIES = (33, 1024, 5000, 32768, 32769, 1048576, 1048577)
TOP_BATCHES = (16384, 1000)

# a case: a ring of `cap` slots holding table `table`, drawn len(batches) times (call numbers 0, 1, ...) with the ring's seed
Case = namedtuple("Case", "cap table batches seed beta")


@functools.lru_cache(maxsize=4)
def priorities(cap, table):
    """the fp32 priority table of a case, seeded by (cap, table); read-only, shared by the tests"""
    rng = np.random.default_rng([cap, TABLES.index(table)])
    if table == "uni":                  # U(0, 3), a fifth of the slots zero
        p = rng.uniform(0.0, 3.0, size=cap)
        p[rng.choice(cap, cap // 5, replace=False)] = 0.0
    elif table == "wide":               # log-uniform over the range (|e| + eps)^alpha produces
        p = np.exp(rng.uniform(np.log(float(P_FLOOR)), np.log(3.0), size=cap))
    elif table == "heavy":              # the floor everywhere, one slot in a thousand (at least one) at the top
        p = np.full(cap, P_FLOOR)
        p[rng.choice(cap, max(1, cap // 1000), replace=False)] = P_HEAVY
    elif table == "endzeros":           # zero children at both ends of nodes: the first 40 slots (a quarter of a small ring) and the last third
        p = rng.uniform(0.1, 3.0, size=cap)
        p[:min(40, cap // 4)] = 0.0
        p[cap - cap // 3:] = 0.0
    elif table == "one":                # a single positive slot
        p = np.zeros(cap)
        p[2 * cap // 3] = 1.75
    elif table == "empty":
        p = np.zeros(cap)
    else:
        raise KeyError(table)
    p = p.astype(np.float32)
    p.setflags(write=False)
    return p


def _table():
    t = {}
    for ci, cap in enumerate(CAPACITIES):
        for ti, table in enumerate(TABLES):
            sets = _TRIPLES if cap in FULL_BATCH_SET else (_PAIRS[(ci + ti) % len(_PAIRS)],)
            for batches in sets:
                # beta = 0.4 is the workload's; heavy runs a large exponent instead (weights down to (P_FLOOR / P_HEAVY)^2 ~ 1e-4)
                beta = 2.0 if table == "heavy" else 0.4
                name = f"{cap}_{table}_b{'-'.join(str(b) for b in batches)}"
                t[name] = Case(cap, table, batches, 0xFEED00 + ti, beta)
    for cap in TOP_CAPACITIES:
        for table in ("uni", "endzeros"):
            t[f"{cap}_{table}_top"] = Case(cap, table, TOP_BATCHES, TOP_SEED, 0.4)
    return t


def reaches_top(batch, r):
    """whether the stratum (batch - 1 + r) of a draw rounds up to the batch size in fp32, so that u = batch * fl(total / batch)"""
    return bool(np.float32(batch - 1) + np.float32(r) == np.float32(batch))


CASES = _table()
