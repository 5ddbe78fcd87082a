"""The prioritized-replay oracle (oracle/xq_oracle_ext.c: radix-32 fp32 sum tree, stratified descent, importance weights) against the plain
fp64 reference of tests/per_ref.py on every case of tests/per_edge_cases.py (not gpu), and the negative control of that reference.

The device is compared with the oracle bit for bit (tests/test_per_shape_edges_gpu.py); this file is what ties the oracle — the
definition both restate — to proportional sampling itself: every draw's mass inside the cumulative interval of its slot up to the fp32
roundings (per_ref.slack_ceiling, derived; per_ref.SLACK_REGRESSION, 2 x measured here), the root total, the weights.

Negative control: check_draw must reject a wrong sampler for the reason it is wrong.
    shift        every slot one leaf further                                   rejected: "slack" (the mass is a leaf's width outside)
    last_child   falling off a node's end takes child 31, not the last > 0     rejected: "eligible" (a zero-priority slot at the top)
    first_leaf   ... takes the last child > 0 but restarts below it at u = 0   rejected: "slack" — the rule this project had; the
                 mass at the top of the range landed on the FIRST leaf of the last subtree, up to 1.7e7 x 2^-24 total away
    table_max    weights normalised by the table's largest weight, not the batch's   rejected: "weights"
    raw          weights left unnormalised                                     rejected: "weights"
    capacity     `capacity` in place of the eligible count in the weight       NOT rejected, by this or any check of what a draw returns:
                 (N p / total)^-beta over its batch maximum does not depend on N, so the mutant is equivalent on the normalised
                 weights, the only ones that leave the library.  The test holds it to equality instead of claiming a rejection;
                 table_max stands beside it as the weight defect that does bite.  (N matters through N = 0 alone: 0^-beta = inf, and
                 inf / inf = NaN — what a one-slot ring gave before its leaf was counted.)
"""
import ctypes as C
import functools

import numpy as np
import pytest

import per_edge_cases as pc
import per_ref as pr
import xqoracle as xo

PF = C.POINTER(C.c_float)


def oracle_tree(prio):
    tree = xo.per_build(prio)
    return tree, float(xo.lib().xqo_per_total(tree.ctypes.data_as(PF), len(prio)))


def oracle_draw(tree, c, call, n_el):
    """the oracle's draw as the library returns one: slots and w / max w in fp32"""
    slots, w_raw, wmax = xo.per_sample(tree, c.cap, c.batches[call], c.seed, call, n_el, c.beta)
    return slots, w_raw / np.float32(wmax), w_raw, wmax


@functools.lru_cache(maxsize=None)
def oracle_figures(name):
    """runs the oracle on a case and check_draw on each of its draws with both limits -> (worst slack, worst weight error)"""
    c = pc.CASES[name]
    prio = pc.priorities(c.cap, c.table)
    _, total, n_el, mx = pr.cdf(prio)
    tree, root = oracle_tree(prio)
    assert abs(root - total) <= pr.total_rtol(c.cap) * total, (root, total)
    assert n_el == int((tree[:c.cap] > 0).sum()) and mx == float(tree[:c.cap].max())        # the reference's statistics: exact
    assert not tree[c.cap:(c.cap + 31) // 32 * 32].any()                                      # padding never carries mass
    slack = w_err = 0.0
    for call, batch in enumerate(c.batches):
        slots, w, _, _ = oracle_draw(tree, c, call, n_el)
        got = pr.check_draw(prio, slots, w, batch, c.seed, call, c.beta, pr.slack_limits(c.cap))
        slack, w_err = max(slack, got["slack"]), max(w_err, got["w_err"])
    print(f"{name}: slack {slack:.3f} of {pr.slack_limits(c.cap)}, weight error {w_err:.3g}, root {abs(root - total) / (pr.ULP * total) if total else 0:.2f} x 2^-24")
    return slack, w_err


@pytest.mark.parametrize("name", list(pc.CASES))
def test_oracle_draws_pass_the_reference_on_every_case(name):
    oracle_figures(name)


def test_table_covers_every_capacity_batch_and_priority_table():
    caps = {c.cap for c in pc.CASES.values()}
    assert caps == set(pc.CAPACITIES)
    for cap in pc.CAPACITIES:
        seen = {b for c in pc.CASES.values() if c.cap == cap and c.seed != pc.TOP_SEED for b in c.batches}
        assert seen == set(pc.BATCHES) if cap in pc.FULL_BATCH_SET else len(seen) >= 2, (cap, seen)
        assert {c.table for c in pc.CASES.values() if c.cap == cap} == set(pc.TABLES)
    assert [len(pr.level_sizes(c)) for c in pc.CAPACITIES] == [1, 2, 2, 2, 3, 3, 4, 4, 4, 5, 5, 6, 6]
    assert pr.level_sizes(1048577) == [1048577, 32769, 1025, 33, 2, 1] and pr.level_sizes(2097153)[1] == 65537
    # duplicates are certain somewhere at every capacity below the largest batch
    assert all(max(c.batches) >= 1000 for c in pc.CASES.values())


def test_measured_figures_are_the_recorded_ones():
    """per_ref's regression limits are 2 x these maxima; a case table that moves them must move the constants (and profiles/NOTES.md)"""
    figs = [oracle_figures(name) for name in pc.CASES]
    slack, w_err = max(f[0] for f in figs), max(f[1] for f in figs)
    print("worst slack", slack, "worst weight error", w_err)
    assert slack <= pr.SLACK_MEASURED_CPU and slack > 0.5 * pr.SLACK_MEASURED_CPU
    assert w_err <= pr.W_MEASURED_CPU and w_err > 0.5 * pr.W_MEASURED_CPU
    assert pr.SLACK_REGRESSION == 2 * pr.SLACK_MEASURED_CPU and pr.SLACK_REGRESSION < pr.slack_ceiling(2)


def test_top_cases_reach_the_top_of_the_range():
    """call 0 of every `top` case: the last stratum rounds up to the batch size, u is the fp32 total itself, and the draw is the LAST slot
    with a positive priority"""
    r = pr.masses(pc.TOP_BATCHES[0], pc.TOP_SEED, 0, float(pc.TOP_BATCHES[0]))[-1] - (pc.TOP_BATCHES[0] - 1)
    assert pc.reaches_top(pc.TOP_BATCHES[0], r)
    for name, c in pc.CASES.items():
        if c.seed != pc.TOP_SEED:
            continue
        prio = pc.priorities(c.cap, c.table)
        tree, root = oracle_tree(prio)
        slots = oracle_draw(tree, c, 0, pr.cdf(prio)[2])[0]
        assert slots[-1] == np.nonzero(prio > 0)[0][-1], name
        assert xo.lib().xqo_per_descend(tree.ctypes.data_as(PF), c.cap, C.c_float(root)) == slots[-1]


# ---- negative control ------------------------------------------------------------------------------------------------------------------
def descend(tree, cap, u, fall_off):
    """the oracle's descent restated on its tree, with the rule for a mass that falls off a node's end as a parameter:
    "oracle" (last child > 0, then the top of the range below), "last_child" (child 31), "first_leaf" (last child > 0, then u = 0)"""
    n = pr.level_sizes(cap)
    off = np.concatenate([[0], np.cumsum([(k + 31) // 32 * 32 for k in n])])
    u, node = np.float32(u), 0
    for lv in range(len(n) - 2, -1, -1):
        v = tree[off[lv] + node * 32: off[lv] + node * 32 + 32]
        pick = -1
        for q in range(32):
            if u < v[q]:
                pick = q
                break
            u = np.float32(u - v[q])
        if pick < 0:
            pos = np.nonzero(v > 0)[0]
            pick = 31 if fall_off == "last_child" else (int(pos[-1]) if len(pos) else 0)
            u = np.float32(0.0 if fall_off == "first_leaf" else np.finfo(np.float32).max)
        node = node * 32 + pick
    return node


def _top_draw(name, fall_off):
    """call 0 of a `top` case; its last 32 draws come from `descend` with the given rule"""
    c = pc.CASES[name]
    prio = pc.priorities(c.cap, c.table)
    tree, root = oracle_tree(prio)
    batch = c.batches[0]
    slots, w, _, _ = oracle_draw(tree, c, 0, pr.cdf(prio)[2])
    seg = np.float32(root) / np.float32(batch)
    r = (pr.masses(batch, c.seed, 0, float(batch)) - np.arange(batch)).astype(np.float32)        # exact: 24-bit fractions
    slots = slots.copy()
    for k in range(batch - 32, batch):
        slots[k] = descend(tree, c.cap, (np.float32(k) + r[k]) * seg, fall_off)
    return c, prio, slots, w, batch


def _case(cap, table):
    """the first case of the table with that capacity and priority table"""
    return next(c for c in pc.CASES.values() if (c.cap, c.table) == (cap, table) and c.seed != pc.TOP_SEED)


def _rejected(field, prio, slots, w, c, call=0):
    with pytest.raises(pr.DrawMismatch) as e:
        pr.check_draw(prio, slots, w, c.batches[call], c.seed, call, c.beta, pr.slack_limits(c.cap))
    assert e.value.field == field, str(e.value)
    return str(e.value)


def test_restated_descent_is_the_oracles():
    for name in ("1024_endzeros_top", "5000_uni_top"):
        c, prio, slots, w, batch = _top_draw(name, "oracle")
        assert np.array_equal(slots, oracle_draw(oracle_tree(prio)[0], c, 0, pr.cdf(prio)[2])[0])
        pr.check_draw(prio, slots, w, batch, c.seed, 0, c.beta, pr.slack_limits(c.cap))


def test_shifted_slots_are_rejected():
    c = _case(1025, "wide")
    prio = pc.priorities(c.cap, c.table)
    tree, _ = oracle_tree(prio)
    slots, w, _, _ = oracle_draw(tree, c, 1, c.cap)
    shifted = np.minimum(slots + 1, c.cap - 1)
    w_shifted = pr.weights(prio, shifted, c.beta)                       # (weights that fit the shifted slots: only the slots are wrong)
    assert "misses its interval" in _rejected("slack", prio, shifted, w_shifted, c, call=1)


def test_last_child_instead_of_last_positive_child_is_rejected():
    """1024 slots are 32 full nodes; `endzeros` empties the last ten of them, so child 31 of the root leads to zero priorities"""
    c, prio, slots, w, _ = _top_draw("1024_endzeros_top", "last_child")
    assert slots[-1] == 1023 and prio[1023] == 0
    assert "zero-priority" in _rejected("eligible", prio, slots, w, c)


def test_restarting_at_zero_below_a_fall_off_is_rejected():
    """the rule the oracle and the device had: the top of the range sampled the first leaf of the last subtree"""
    for name in ("1024_endzeros_top", "1048576_uni_top"):
        c, prio, slots, w, _ = _top_draw(name, "first_leaf")
        assert slots[-1] < np.nonzero(prio > 0)[0][-1] and prio[slots[-1]] > 0
        w = pr.weights(prio, slots, c.beta)
        assert "draw 16383" in _rejected("slack", prio, slots, w, c)


def test_wrong_weights_are_rejected_and_the_equivalent_mutant_is_named():
    c = _case(5000, "uni")
    prio = pc.priorities(c.cap, c.table)
    _, total, n_el, _ = pr.cdf(prio)
    assert n_el < c.cap
    tree, _ = oracle_tree(prio)
    slots, w, w_raw, wmax = oracle_draw(tree, c, 1, n_el)
    pr.check_draw(prio, slots, w, c.batches[1], c.seed, 1, c.beta, pr.slack_limits(c.cap))
    # unnormalised
    assert wmax > 1.5
    _rejected("weights", prio, slots, w_raw, c, call=1)
    # normalised by the table's largest weight instead of the batch's: the batch does not hold the table's smallest priority
    table_max = np.float32((n_el * float(prio[prio > 0].min()) / total) ** -c.beta)
    assert table_max > 1.05 * wmax
    _rejected("weights", prio, slots, w_raw / table_max, c, call=1)
    # `capacity` in place of the eligible count: another raw weight, the same normalised one (see the module docstring)
    _, w_cap, w_cap_raw, _ = oracle_draw(tree, c, 1, c.cap)
    assert np.abs(w_cap_raw / w_raw - (c.cap / n_el) ** -c.beta).max() < 1e-6 and (c.cap / n_el) ** -c.beta < 0.95
    pr.check_draw(prio, slots, w_cap, c.batches[1], c.seed, 1, c.beta, pr.slack_limits(c.cap))
    assert np.abs(w_cap - w).max() <= 2 * pr.W_MEASURED_CPU


def test_empty_table_and_one_slot_ring_give_the_documented_results():
    for cap in (1, 33, 5000):
        prio = pc.priorities(cap, "empty")
        tree, root = oracle_tree(prio)
        slots, w_raw, wmax = xo.per_sample(tree, cap, 65, 7, 0, 0, 0.4)
        assert root == 0 and not slots.any() and np.array_equal(w_raw, np.ones(65, np.float32)) and wmax == 1.0
    # one slot, one positive priority, counted: weight (1 * p / p)^-beta = 1
    tree, root = oracle_tree(np.array([0.37], np.float32))
    slots, w_raw, wmax = xo.per_sample(tree, 1, 8, 7, 0, 1, 0.4)
    assert root == np.float32(0.37) and not slots.any() and np.array_equal(w_raw, np.ones(8, np.float32)) and wmax == 1.0
