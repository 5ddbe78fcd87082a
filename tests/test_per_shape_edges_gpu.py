"""The prioritized-replay kernels (csrc/xq_replay.hip: per_level_kernel, per_upper_kernel, per_fill_kernel, per_sample_kernel) on every
case of tests/per_edge_cases.py — `pytest -m gpu`.

Host code and kernel loops flip with the ring's capacity: no level kernel at one slot, no upper levels up to 32, the strided loops of
per_upper_kernel beyond 1 M and 2 M slots.  Each case sets a priority table, rebuilds the tree and draws two or three minibatches.  The
tree's root is the oracle's bit for bit and the fp64 total within per_ref.total_rtol; the statistics are exact; every draw equals the
oracle's slot for slot and passes per_ref.check_draw on its own — slots eligible, every mass inside its slot's fp64 cumulative interval
within both limits of per_ref.slack_limits, strata in order, weights within per_ref.W_TOL.  Then retire windows that wrap, beta = 0, and
prioritized TD steps at the edges tests/test_config5_gpu.py leaves out.  Figures per capacity on an MI355X: profiles/NOTES.md
("Prioritized replay against fp64").
"""
import ctypes as C

import numpy as np
import pytest

import per_edge_cases as pc
import per_ref as pr
import xqoracle as xo
from test_config5_gpu import _filled_ring, oracle_update
from test_dqn_gpu import PTOL, make_net

pytestmark = pytest.mark.gpu

PF = C.POINTER(C.c_float)
SMALL_NET = [1260, 64, 64, 8100]


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def trace(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "ref_trace.npz"))


def check_tree(rp, prio):
    """the rebuilt tree's statistics against the oracle (same bits) and the fp64 table; returns (oracle tree, eligible count)"""
    cap = len(prio)
    _, total, n_el, mx = pr.cdf(prio)
    tree = xo.per_build(prio)
    st = rp.per_stats()
    assert st["total"] == float(xo.lib().xqo_per_total(tree.ctypes.data_as(PF), cap))
    assert abs(st["total"] - total) <= pr.total_rtol(cap) * total, (st["total"], total)
    assert st["n_eligible"] == n_el
    assert st["max_priority"] == max(1.0, mx)            # the running maximum: 1 at start, then the largest priority ever assigned
    return tree, n_el


def check_draw(rp, prio, tree, n_el, batch, seed, call, beta):
    """one draw of the ring against the oracle's (slot for slot) and, on its own, against the fp64 reference"""
    cap = len(prio)
    slots, w = rp.sample_prioritized(batch)
    want_slots, _, _ = xo.per_sample(tree, cap, batch, seed, call, n_el, beta)
    fig = pr.check_draw(prio, slots, w, batch, seed, call, beta, pr.slack_limits(cap))
    assert np.array_equal(slots, want_slots)
    assert abs(float(w.max()) - 1.0) < 1e-6
    return fig


@pytest.mark.parametrize("name", list(pc.CASES))
def test_tree_and_draws_match_oracle_and_fp64_reference(xq, name):
    c = pc.CASES[name]
    prio = pc.priorities(c.cap, c.table)
    rp = xq.ReplayBuffer(c.cap, seed=c.seed)
    try:
        rp.enable_per(0.6, c.beta, 1e-3)
        rp.set_priorities(prio)
        rp.per_rebuild()
        tree, n_el = check_tree(rp, prio)
        figs = [check_draw(rp, prio, tree, n_el, batch, c.seed, call, c.beta) for call, batch in enumerate(c.batches)]
        print(f"{name}: slack {max(f['slack'] for f in figs):.3f} of {pr.slack_limits(c.cap)}, weight error {max(f['w_err'] for f in figs):.3g}")
    finally:
        rp.close()


@pytest.mark.parametrize("cap", pc.FULL_BATCH_SET)
def test_retire_windows_leave_the_tree_and_the_draws(xq, cap):
    """per_rebuild(cap - 10, 25) wraps past the end of the ring: exactly those 25 slots lose their priority, the next draw (the second
    from this ring, after a draw nothing consumed) avoids them and is a right draw of the retired table; retiring everything leaves the
    empty ring's documented result"""
    seed, beta = 0xFEED77, 0.4
    prio = pc.priorities(cap, "uni")
    rp = xq.ReplayBuffer(cap, seed=seed)
    try:
        rp.enable_per(0.6, beta, 1e-3)
        rp.set_priorities(prio)
        rp.per_rebuild()
        tree, n_el = check_tree(rp, prio)
        check_draw(rp, prio, tree, n_el, 1000, seed, 0, beta)
        retired = np.arange(cap - 10, cap + 15) % cap
        want = prio.copy()
        want[retired] = 0.0
        assert (prio[retired] > 0).sum() >= 10
        rp.per_rebuild(cap - 10, 25)
        assert np.array_equal(rp.get_priorities(), want)
        tree, n_el = check_tree(rp, want)
        for call, batch in ((1, 16384), (2, 65)):
            check_draw(rp, want, tree, n_el, batch, seed, call, beta)
        slots, _ = rp.sample_prioritized(4096)
        assert not np.isin(slots, retired).any()
        rp.per_rebuild(0, cap)
        assert not rp.get_priorities().any()
        st = rp.per_stats()
        assert st["total"] == 0.0 and st["n_eligible"] == 0
        slots, w = rp.sample_prioritized(1000)
        assert not slots.any() and np.array_equal(w, np.ones(1000, np.float32))
    finally:
        rp.close()


@pytest.mark.parametrize("cap,table", [(1, "one"), (32, "wide"), (5000, "wide"), (1048577, "heavy")])
def test_beta_zero_gives_unit_weights(xq, cap, table):
    prio = pc.priorities(cap, table)
    rp = xq.ReplayBuffer(cap, seed=3)
    try:
        rp.enable_per(0.6, 0.0, 1e-3)
        rp.set_priorities(prio)
        rp.per_rebuild()
        for batch in (65, 1000):
            slots, w = rp.sample_prioritized(batch)
            assert (prio[slots] > 0).all() and np.array_equal(w, np.ones(batch, np.float32))
    finally:
        rp.close()


# ---- prioritized TD steps -------------------------------------------------------------------------------------------------------------
def _td_step(xq, rp, batch, seed):
    """one Double-DQN step of SMALL_NET on a prioritized draw of the ring -> (slots, weights, handle, start parameters, target parameters)"""
    d, w, b = make_net(xq, SMALL_NET, seed=seed)
    wt, bt = xo.init_weights(SMALL_NET, seed + 1)
    d.set_params(wt, bt, net=1)
    slots, wts = rp.sample_prioritized(batch)
    d.td_grads_replay(rp, batch, td_net=xq._capi.TD_DOUBLE, mode=0)
    d.apply_grads(0.05, 1.0 / batch)
    return slots, wts, d, (w, b), (wt, bt)


def test_prioritized_td_step_with_every_slot_drawn_several_times(xq, trace):
    """batch 160 from 40 transitions: every slot is drawn at least twice, so every priority is written by several samples (with the same
    value).  Parameters, written-back priorities and the running maximum against the fp64 step, with the tolerances of
    tests/test_config5_gpu.py::test_prioritized_td_step_weights_and_priorities."""
    cap, n, batch = 64, 40, 160
    rp, (S, A, R, D, S2) = _filled_ring(xq, trace, cap, n, seed=4)
    prio = np.random.default_rng(5).uniform(1.0, 2.0, size=n).astype(np.float32)          # shares of 160 draws: all above 2
    rp.set_priorities(prio)
    rp.per_rebuild()
    slots, wts, d, (w, b), (wt, bt) = _td_step(xq, rp, batch, seed=15)
    assert np.bincount(slots, minlength=cap)[:n].min() >= 2 and slots.max() < n
    full = np.concatenate([prio, np.zeros(cap - n, np.float32)])
    pr.check_draw(full, slots, wts, batch, 0xFEED + 4, 0, 0.4, pr.slack_limits(cap))
    want_w, want_b, want_q, want_y, _ = oracle_update(SMALL_NET, w, b, wt, bt, S[slots], A[slots], R[slots], D[slots], S2[slots], 0.99,
                                                      0.05, 1.0 / batch, 0, 2, weights=wts)
    got_w, got_b = d.get_params()
    assert np.abs(got_w - want_w).max() < PTOL and np.abs(got_b - want_b).max() < PTOL
    assert np.abs(want_w - w).max() > 1e-5
    p2 = rp.get_priorities()
    want_p = np.zeros(cap)
    for s, q, y in zip(slots, want_q, want_y):
        want_p[s] = (abs(q - y) + 1e-3) ** 0.6
    assert np.allclose(p2[:n], want_p[:n], rtol=2e-3, atol=1e-5)
    assert not p2[n:].any()                                   # never pushed, never drawn: untouched
    rp.per_rebuild()
    assert abs(rp.per_stats()["max_priority"] - max(prio.max(), want_p.max())) < 1e-3
    d.close(); rp.close()


def test_alpha_zero_writes_unit_priorities(xq, trace):
    cap, n, batch = 64, 40, 32
    rp, _ = _filled_ring(xq, trace, cap, n, seed=4, per=(0.0, 0.4, 1e-3))
    prio = np.random.default_rng(6).uniform(1.25, 2.0, size=n).astype(np.float32)
    rp.set_priorities(prio)
    rp.per_rebuild()
    slots, _, d, _, _ = _td_step(xq, rp, batch, seed=15)
    p2 = rp.get_priorities(0, n)
    drawn = np.unique(slots)
    assert 0 < len(drawn) < n
    assert np.array_equal(p2[drawn], np.ones(len(drawn), np.float32))            # (|Q - y| + eps)^0, exactly
    rest = np.setdiff1d(np.arange(n), drawn)
    assert np.array_equal(p2[rest], prio[rest])
    d.close(); rp.close()


def test_one_slot_ring_trains_like_an_unweighted_step(xq, trace):
    """a ring of one slot has no tree level above the leaf: its eligible count is the leaf's own.  (Counted as 0, the raw weight is
    0^-beta = inf and the normalised one inf / inf = NaN: the step then writes NaN into every parameter.)"""
    batch = 8
    rp, (S, A, R, D, S2) = _filled_ring(xq, trace, 1, 1, seed=4, per=(0.6, 0.4, 1e-3))
    rp.per_rebuild()
    st = rp.per_stats()
    assert st["n_eligible"] == 1 and st["total"] == 1.0 and st["max_priority"] == 1.0
    slots, wts, d, (w, b), (wt, bt) = _td_step(xq, rp, batch, seed=15)
    assert not slots.any() and np.array_equal(wts, np.ones(batch, np.float32))
    got_w, got_b = d.get_params()
    assert np.isfinite(got_w).all() and np.isfinite(got_b).all()
    want_w, want_b, _, _, _ = oracle_update(SMALL_NET, w, b, wt, bt, S[slots], A[slots], R[slots], D[slots], S2[slots], 0.99, 0.05,
                                            1.0 / batch, 0, 2)
    assert np.abs(got_w - want_w).max() < PTOL and np.abs(got_b - want_b).max() < PTOL
    assert np.abs(want_w - w).max() > 1e-5
    d.close(); rp.close()
