"""Plain fp64 reference of stratified proportional prioritized sampling, for tests/test_per_ref_cpu.py (the oracle against it) and
tests/test_per_shape_edges_gpu.py (the device against it).  Test infrastructure only.

No tree: the priorities' fp64 cumulative sums.  A draw k of a batch B owns the mass u_k = (k + r_k) * total / B and is right when
u_k lies in the cumulative interval [C[slot - 1], C[slot]] of the slot it returned.  The device (csrc/xq_replay.hip) and the oracle
(oracle/xq_oracle_ext.c) walk a radix-32 fp32 sum tree instead, so their u_k and their partial sums carry fp32 roundings: the chosen
interval may miss the fp64 u_k by a few ulps of the total.  `interval_slack` measures that miss in units of 2^-24 * total; the two
limits below bound it.  Nothing here is shared with the oracle except its Philox (pinned by Random123 known answers in
tests/test_oracle_golden.py::test_philox_known_answers).
"""
import functools

import numpy as np

import xqoracle as xo

ULP = 2.0 ** -24        # the unit of every slack: 2^-24 * total

# ---- limits -----------------------------------------------------------------------------------------------------------------------------
# Regression limit on interval_slack: 2 x the worst slack of the CPU oracle (never the device) against this reference over every case of
# tests/per_edge_cases.py, as printed by tests/test_per_ref_cpu.py::test_oracle_draws_pass_the_reference_on_every_case; per capacity in
# profiles/NOTES.md ("Prioritized replay against fp64").  The factor 2: the maximum over a few thousand roundings moves by well under
# 2 x between seeds.
SLACK_MEASURED_CPU = 3.61       # at 32769 slots; 0 up to 33 slots, 0.33 .. 3.6 above
SLACK_REGRESSION = 2 * SLACK_MEASURED_CPU

# Normalised weights w / max w (values <= 1): the oracle's fp32 weights against weights() below, worst absolute difference over the same
# cases on the CPU, doubled as above; on top of it the rtol the device is held to against the oracle
# (tests/test_config5_gpu.py::test_sum_tree_and_sampler_are_bit_exact: its own powf and one division).  W_TOL, their sum, is the
# bound at w = 1; check_draw applies W_ORACLE_ABS + W_DEVICE_RTOL * w.
W_MEASURED_CPU = 1.31e-7
W_ORACLE_ABS = 2 * W_MEASURED_CPU
W_DEVICE_RTOL = 2e-6
W_TOL = W_ORACLE_ABS + W_DEVICE_RTOL

# Form of the stratum-order check (3) of check_draw: "strict", slots never go backwards.  No relaxed form was needed, and none can be: the
# fp32 u_k is non-decreasing in k (rounding is monotone), a node's walk keeps two masses in order (the same subtractions, rounded
# monotonically), and a mass that falls off a node's end takes the last eligible leaf below that node — no leaf of the node lies behind it.
ORDER_FORM = "strict"


def level_sizes(cap):
    """nodes per level of the radix-32 tree over `cap` leaves, leaves first: 32 children per node up to a single root"""
    n = [int(cap)]
    while n[-1] > 1:
        n.append((n[-1] + 31) // 32)
    return n


def slack_ceiling(cap):
    """Hard ceiling on interval_slack, from the algorithm: every level below the root adds at most 31 sequential fp32 additions to a node
    (31 * 2^-24 relative, so at most 31 * 2^-24 * total on a partial sum) and at most 31 subtractions from u (each rounds by at most
    2^-24 * total); forming u = (k + r) * (total / B) takes 3 roundings.  3 + 62 * (nlv - 1), in units of 2^-24 * total."""
    return 3 + 62 * (len(level_sizes(cap)) - 1)


def total_rtol(cap):
    """the tree's fp32 root against the fp64 total: 31 sequential additions per level below the root"""
    return 31 * (len(level_sizes(cap)) - 1) * ULP


def slack_limits(cap):
    return slack_ceiling(cap), SLACK_REGRESSION


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def cdf(prio):
    """-> (C, total, n_eligible, max): fp64 cumulative sums of the fp32 priorities and the three statistics of the table"""
    prio = np.asarray(prio, dtype=np.float32)
    C = np.cumsum(prio.astype(np.float64))
    return C, float(C[-1]), int((prio > 0).sum()), float(prio.max())


@functools.lru_cache(maxsize=64)
def _strata(batch, seed, call):
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    r = np.array([xo.philox([k, 0, call, 2], key)[0] >> 8 for k in range(batch)], dtype=np.float64) * ULP
    r.setflags(write=False)
    return r


def masses(batch, seed, call, total):
    """u_k = (k + r_k) * total / batch in fp64, r_k = (philox([k, 0, call, 2], seed)[0] >> 8) * 2^-24"""
    return (np.arange(batch, dtype=np.float64) + _strata(int(batch), int(seed), int(call))) * float(total) / batch


def _intervals(C, slots):
    slots = np.asarray(slots, dtype=np.int64)
    lo = np.where(slots > 0, C[np.maximum(slots - 1, 0)], 0.0)
    return lo, C[slots]


def interval_slack(prio, slots, u):
    """for each draw: how far u_k lies outside [C[slot - 1], C[slot]], 0 inside, in units of 2^-24 * total"""
    C, total, _, _ = cdf(prio)
    if total == 0:
        return np.zeros(len(slots))
    lo, hi = _intervals(C, slots)
    return np.maximum(np.maximum(lo - u, u - hi), 0.0) / (ULP * total)


def weights(prio, slots, beta):
    """(n_eligible * p[slot] / total)^-beta in fp64 over its batch maximum; 1 for an empty table (nothing to weigh)"""
    prio = np.asarray(prio, dtype=np.float32)
    _, total, n_el, _ = cdf(prio)
    if total == 0:
        return np.ones(len(slots))
    with np.errstate(divide="ignore"):
        w = (n_el * prio[np.asarray(slots, dtype=np.int64)].astype(np.float64) / total) ** -float(beta)
    return w / w.max()


class DrawMismatch(AssertionError):
    """check_draw's refusal; .field names the property that failed: "range", "eligible", "slack", "order", "weights", "empty" """

    def __init__(self, field, message):
        super().__init__(f"{field}: {message}")
        self.field = field


def check_draw(prio, slots, w, batch, seed, call, beta, slack_limit):
    """A draw (slots, normalised weights w) of `batch` from the table `prio` with the ring's seed and call number.  slack_limit: one
    limit or several (all must hold).  Raises DrawMismatch; returns the figures it measured."""
    prio = np.asarray(prio, dtype=np.float32)
    slots = np.asarray(slots)
    w = np.asarray(w, dtype=np.float64)
    cap = len(prio)
    limit = float(np.min(np.atleast_1d(slack_limit)))
    if slots.shape != (batch,) or w.shape != (batch,):
        raise DrawMismatch("range", f"{slots.shape} slots and {w.shape} weights for a batch of {batch}")
    C, total, n_el, _ = cdf(prio)
    if n_el == 0:                                   # the documented result of an empty table: slot 0, weight 1
        if slots.any() or not np.array_equal(w, np.ones(batch)):
            raise DrawMismatch("empty", "an empty table gives slot 0 with weight 1")
        return dict(slack=0.0, w_err=0.0)
    # 1. real, eligible slots
    if slots.min() < 0 or slots.max() >= cap:
        raise DrawMismatch("range", f"slots {slots.min()} .. {slots.max()} outside [0, {cap})")
    dead = np.nonzero(prio[slots] <= 0)[0]
    if len(dead):
        raise DrawMismatch("eligible", f"{len(dead)} draws of zero-priority slots, first: draw {dead[0]} -> slot {slots[dead[0]]}")
    # 2. every mass inside its slot's cumulative interval, up to the fp32 roundings
    u = masses(batch, seed, call, total)
    slack = interval_slack(prio, slots, u)
    worst = int(np.argmax(slack))
    if slack[worst] > limit:
        raise DrawMismatch("slack", f"draw {worst} -> slot {slots[worst]}: u misses its interval by {slack[worst]:.3g} x 2^-24 total, "
                                    f"limit {limit:.3g}")
    # 3. the strata are increasing, so the slots never go backwards
    back = np.nonzero(np.diff(slots.astype(np.int64)) < 0)[0]
    if len(back):
        raise DrawMismatch("order", f"{len(back)} reversed neighbours, first: draws {back[0]}, {back[0] + 1} -> slots "
                                    f"{slots[back[0]]}, {slots[back[0] + 1]}")
    # 4. importance weights
    want = weights(prio, slots, beta)
    err = np.abs(w - want)
    bad = np.nonzero(~(err <= W_ORACLE_ABS + W_DEVICE_RTOL * want))[0]
    if len(bad):
        raise DrawMismatch("weights", f"{len(bad)} weights off, first: draw {bad[0]} -> {w[bad[0]]!r}, want {want[bad[0]]!r}")
    return dict(slack=float(slack[worst]), w_err=float(err.max()))
