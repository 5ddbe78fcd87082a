"""n-step TD returns from the replay ring (xq_replay_set_n_step, DESIGN.md §4 "n-step returns") on the device: the assembled batch
against tests/nstep_ref.py bit for bit, the TD step on it against the existing step on the reference's transitions bit for bit, off is
off, the prioritized write-back and the hold window, the trainer's windows, refusals, and what the setting survives."""
import json
import subprocess

import numpy as np
import pytest

import batch_ref as br
import nstep_ref as nr
import per_ref as pr
import xqoracle as xo
from test_dqn_gpu import CFG2_NET, make_net
from ring_window_ref import default_range, overlap_window, tree_range

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.97
BATCHES = (1, 63, 64, 65, 257)
PER = (0.6, 0.4, 1e-3)


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def small(xq):
    d, _, _ = make_net(xq, SMALL_NET, seed=3, gamma=GAMMA)
    yield d
    d.close()


def filled(xq, fx, seed=5, per=None):
    """the fixture's transitions pushed in push order (in pieces no larger than the ring)"""
    rp = xq.ReplayBuffer(fx["cap"], seed=seed)
    if per:
        rp.enable_per(*per)
    for t in range(0, fx["pushes"], fx["cap"]):
        e = min(t + fx["cap"], fx["pushes"])
        rp.push(fx["push_S"][t:e], fx["push_A"][t:e], fx["push_R"][t:e], fx["push_D"][t:e], fx["push_S2"][t:e])
    assert rp.stats() == (fx["size"], fx["cap"], fx["pushes"])
    return rp


def reference(fx, slots, n, gamma=GAMMA, first=None, count=None):
    if first is None:
        first, count = nr.readable(fx["cap"], fx["size"], fx["write_pos"])
    return nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], gamma, first, count)


def assert_assembled(got, ref):
    assert np.array_equal(got["reward"].view(np.uint32), ref["reward"].view(np.uint32))
    for k in ("done", "steps", "first_slot", "last_slot", "action"):
        assert np.array_equal(got[k], ref[k]), k


# ---- 1. assembly is exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(nr.FIXTURES))
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_assembled_batch_equals_the_reference(xq, small, name, n):
    fx = nr.named_fixture(name)
    rp = filled(xq, fx)
    try:
        rp.set_n_step(n, fx["stride"])
        assert rp.n_step == (n, fx["stride"])
        seen = set()
        for batch in BATCHES:
            slots = rp.sample(batch)
            small.td_grads_replay(rp, batch)
            small.apply_grads(0.0, 1.0)
            ref = reference(fx, slots, n)
            assert_assembled(small.last_n_step(batch), ref)
            seen |= set(ref["cls"])
        small.td_grads_replay(rp, 0)                                  # the identity over the filled part
        ref = reference(fx, nr.filled_slots(fx), n)
        assert_assembled(small.last_n_step(fx["size"]), ref)
        seen |= set(ref["cls"])
        if n == nr.FIXTURES[name][3]:
            assert set(nr.classes(n)) <= seen
        small.apply_grads(0.0, 1.0)
    finally:
        rp.close()


# ---- 2. the step is the existing step on the assembled batch ----------------------------------------------------------------------
@pytest.mark.parametrize("sizes,batch,extras", [(SMALL_NET, 65, False), (CFG2_NET, 1024, False), (CFG2_NET, 1024, True)])
def test_step_is_the_existing_step_on_the_assembled_batch(xq, sizes, batch, extras):
    n, lr = 3, 0.05
    fx = nr.fixture(300, 4, 420, seed=11)
    rp = filled(xq, fx)
    disc = nr.discounts(GAMMA, n)
    a, w, b = make_net(xq, sizes, seed=8, gamma=GAMMA)
    bq, _, _ = make_net(xq, sizes, seed=8, gamma=float(disc[n]))
    try:
        for d in (a, bq):
            if extras:
                d.set_optimizer("adam")
                d.set_td_loss("huber", 0.05)
                d.set_grad_clip(1.0)
        rp.set_n_step(n, fx["stride"])
        slots = rp.sample(batch)
        a.td_grads_replay(rp, batch)
        a.apply_grads(lr, 1.0 / batch)
        qa, ya = a.last_td_values(batch)
        ref = reference(fx, slots, n)
        assert_assembled(a.last_n_step(batch), ref)
        assert ref["dead"].any() and (~ref["dead"]).sum() > batch // 2 and (ref["steps"] == n).any()
        S, A, R, D, S2 = nr.staged(fx, ref)
        qb, yb = bq.td_update(S, S2, A, R, D, learning_rate=lr, grad_scale=1.0 / batch)
        assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32)) and np.array_equal(ya.view(np.uint32), yb.view(np.uint32))
        (wa, ba), (wb, bb) = a.get_params(), bq.get_params()
        assert np.array_equal(wa, wb) and np.array_equal(ba, bb)
        assert np.abs(wa - w).max() > 0
        # and the discount is disc_n, not gamma: a live row that is not done has y - R = disc_n tanh(max), |.| <= disc_n
        live = ~ref["dead"] & (ref["done"] == 0)
        assert live.any() and (np.abs(ya[live].astype(np.float64) - ref["reward"][live]) <= float(disc[n]) * (1 + 1e-6)).all()
    finally:
        a.close(); bq.close(); rp.close()


# ---- 3. off is off ------------------------------------------------------------------------------------------------------------------
def test_n_step_one_is_a_ring_that_was_never_asked(xq):
    fx = nr.named_fixture("wrapped37")
    never, asked = filled(xq, fx), filled(xq, fx)
    asked.set_n_step(3, 4)
    asked.set_n_step(1, 4)
    da, _, _ = make_net(xq, SMALL_NET, seed=4, gamma=GAMMA)
    db, _, _ = make_net(xq, SMALL_NET, seed=4, gamma=GAMMA)
    try:
        for d, rp in ((da, never), (db, asked)):
            d.kernel_stats(2)
            for _ in range(3):
                rp.sample(65)
                d.td_grads_replay(rp, 65)
                d.apply_grads(0.05, 1.0 / 65)
        sa, sb = da.kernel_stats(), db.kernel_stats()
        assert [(s["name"], s["launches"]) for s in sa] == [(s["name"], s["launches"]) for s in sb]
        assert not any(s["name"] in ("nstep_assemble", "per_writeback") for s in sb)
        (wa, ba), (wb, bb) = da.get_params(), db.get_params()
        assert np.array_equal(wa, wb) and np.array_equal(ba, bb)
        qa, qb = da.last_td_values(65), db.last_td_values(65)
        assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
        with pytest.raises(xq.XqError) as e:
            db.last_n_step(1)
        assert e.value.code == 2
        # ... and switched on, the bracket is there: one launch per step
        asked.set_n_step(3, 4)
        asked.sample(65)
        db.td_grads_replay(asked, 65)
        db.apply_grads(0.0, 1.0)
        st = {s["name"]: s for s in db.kernel_stats()}
        assert st["nstep_assemble"]["launches"] == 1 and st["nstep_assemble"]["exact"] == 1
        # raw pointers are never affected: a host-batch step is not an n-step one
        db.td_update(fx["S"][:8], fx["S2"][:8], fx["A"][:8], fx["R"][:8], fx["D"][:8], learning_rate=0.0)
        with pytest.raises(xq.XqError):
            db.last_n_step(1)
    finally:
        da.close(); db.close(); never.close(); asked.close()


# ---- 4. prioritized -----------------------------------------------------------------------------------------------------------------
def test_prioritized_n_step_td_step_and_its_priorities(xq):
    """a Double-DQN step of the small net on a prioritized draw with n_step = 3, against tests/batch_ref.py on the assembled transitions
    with gamma = disc_3 (the bounds of tests/test_td_full_size_gpu.py's prioritized cases); dead rows keep their priority bit for bit"""
    n, batch, lr = 3, 160, 0.05
    scale = 16.0 / batch
    fx = nr.named_fixture("wrapped37")
    rp = filled(xq, fx, per=PER)
    d, _, _ = make_net(xq, SMALL_NET, seed=15, gamma=GAMMA)
    try:
        wt, _ = xo.init_weights(SMALL_NET, 16)
        bt = np.random.default_rng(17).uniform(-0.05, 0.05, size=xo.nn_counts(SMALL_NET)[1])
        d.set_params(wt, bt, net=1)
        w0, b0 = d.get_params()
        wt0, bt0 = d.get_params(1)
        prio = np.random.default_rng(5).uniform(1.0, 2.0, size=fx["cap"]).astype(np.float32)
        rp.set_priorities(prio)
        rp.per_rebuild()
        rp.set_n_step(n, fx["stride"])
        slots, weights = rp.sample_prioritized(batch)
        d.td_grads_replay(rp, batch, td_net=xq._capi.TD_DOUBLE, mode=0)
        d.apply_grads(lr, scale)
        q_dev, y_dev = d.last_td_values(batch)
        new_w, new_b = d.get_params()
        ref = reference(fx, slots, n)
        assert_assembled(d.last_n_step(batch), ref)
        assert ref["dead"].any() and set(ref["cls"]) >= {"full", "incomplete", "empty_mid", "empty0"}
        S, A, R, D, S2 = nr.staged(fx, ref)
        disc3 = float(nr.discounts(GAMMA, n)[n])
        net, tnet = br.Net(SMALL_NET, w0, b0, br.PRECISION_F32), br.Net(SMALL_NET, wt0, bt0, br.PRECISION_F32)
        f = br.forward(net, S, S2, A, R, D, disc3, 2, br.PRECISION_F32, target=tnet)
        _, y_use = br.check_q_y(f, q_dev, y_dev, br.PRECISION_F32)
        u = br.accumulate(net, f, br.backward(net, f, 0, br.PRECISION_F32, weights, y=y_use), br.PRECISION_F32)
        br.check_update(net, u, f, new_w, new_b, lr, scale, br.PRECISION_F32)
        p2 = rp.get_priorities(0, fx["cap"])
        live = ~ref["dead"]
        p_dev = (np.abs(q_dev.astype(np.float64) - y_dev) + PER[2]) ** PER[0]
        assert np.allclose(p2[slots[live]], p_dev[live], rtol=2e-5, atol=0)
        assert np.abs(br.priorities(f, PER[2], PER[0], y=y_use)[live] ** (1 / PER[0]) - p_dev[live] ** (1 / PER[0])).max() < 2 * br.QTOL
        untouched = np.setdiff1d(np.arange(fx["cap"]), slots[live])
        assert len(np.intersect1d(untouched, slots[~live])) > 0                     # dead rows that were drawn: same bits as before
        assert np.array_equal(p2[untouched].view(np.uint32), prio[untouched].view(np.uint32))
        rp.per_rebuild()
        assert rp.per_stats()["max_priority"] == max(float(prio.max()), float(p2.max()))
    finally:
        d.close(); rp.close()


@pytest.mark.parametrize("cap", [37, 5000])
def test_rebuild_with_a_hold_window(xq, cap):
    """held slots are never drawn and are not eligible, the live table is unchanged; a later rebuild without the hold brings them back;
    a hold of 0 is today's rebuild, draw for draw"""
    seed, beta = 0xFEED + 9, 0.4
    prio = np.random.default_rng(cap).uniform(0.5, 2.0, size=cap).astype(np.float32)
    plain, rp = xq.ReplayBuffer(cap, seed=seed), xq.ReplayBuffer(cap, seed=seed)
    try:
        for r in (plain, rp):
            r.enable_per(PER[0], beta, PER[2])
            r.set_priorities(prio)
        plain.per_rebuild()
        xq._capi.call("xq_replay_per_rebuild_hold", rp.handle, 0, 0, 5, 0)                # a hold of 0, through the new entry point
        assert rp.per_stats() == plain.per_stats()
        s0, w0 = plain.sample_prioritized(257)
        s1, w1 = rp.sample_prioritized(257)
        assert np.array_equal(s0, s1) and np.array_equal(w0, w1)
        hold_start, hold_count = cap - 6, 11                                             # wraps past the end of the ring
        held = np.arange(hold_start, hold_start + hold_count) % cap
        want = prio.copy(); want[held] = 0.0
        rp.per_rebuild(0, 0, hold_start, hold_count)
        assert np.array_equal(rp.get_priorities(), prio)                                 # the live table keeps every value
        _, total, n_el, _ = pr.cdf(want)
        st = rp.per_stats()
        assert st["n_eligible"] == n_el == cap - hold_count
        assert abs(st["total"] - total) <= pr.total_rtol(cap) * total
        tree = xo.per_build(want)
        for call, batch in ((1, 4096), (2, 65)):
            slots, w = rp.sample_prioritized(batch)
            want_slots, _, _ = xo.per_sample(tree, cap, batch, seed, call, n_el, beta)
            assert np.array_equal(slots, want_slots) and not np.isin(slots, held).any()
        rp.per_rebuild(hold_start, 3, (hold_start + 3) % cap, 2)                         # retire 3 of them, hold 2 more, release the rest
        want = prio.copy(); want[held[:3]] = 0.0
        assert np.array_equal(rp.get_priorities(), want)
        want[held[3:5]] = 0.0
        assert rp.per_stats()["n_eligible"] == cap - 5
        slots, _ = rp.sample_prioritized(4096)
        assert not np.isin(slots, held[:5]).any() and (np.isin(held[5:], slots).all() or cap > 64)
    finally:
        plain.close(); rp.close()


# ---- 5. trainer -----------------------------------------------------------------------------------------------------------------------
def ring_arrays(rp, cap):
    A, R, D = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.uint8)
    for s in range(cap):
        _, A[s], R[s], D[s], _ = rp.get(s)
    return A, R, D


@pytest.mark.parametrize("overlap,plies,versus", [(0, 1, False), (1, 1, False), (0, 2, False), (1, 2, True), (0, 1, True)])
def test_trainer_assembles_complete_chains(xq, overlap, plies, versus):
    """64 games, a ring that is no multiple of 64 and wraps several times, n_step = 3: after each learn_grads the assembled batch is
    the reference walked over the ring's contents with the trainer's documented windows; from iteration 3 on no row is dead for an
    incomplete chain (the sample window leaves out the newest 2 x 64 slots)"""
    G, cap, mb, n, iters = 64, 64 * 7 + 37, 96, 3, 12
    cfg = xq.TrainerConfig(n_games=G, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.3, replay_capacity=cap,
                           minibatch=mb, td_net=1, target_sync_interval=3, seed=21, collects_per_update=plies, overlap_collect=overlap)
    t = xq.Trainer(cfg)
    try:
        if versus:
            t.set_opponent("random")
        t.set_n_step(n)
        assert t.replay.n_step == (n, G)
        m = plies * G
        incomplete_late = 0
        for it in range(iters):
            if overlap:
                size, _, total = t.replay.stats()
                first, count = overlap_window(size, total, cap, m)
                t.learn_grads()
                size2, _, total2 = t.replay.stats()
                if total2 != total:                                  # nothing older than this iteration's plies: it played them first
                    first, count = default_range(size2, total2, cap)
            else:
                for _ in range(plies):
                    t.collect()
                size, _, total = t.replay.stats()
                first, count = default_range(size, total, cap)
                t.learn_grads()
            got = t.dqn.last_n_step(mb)
            A, R, D = ring_arrays(t.replay, cap)
            ref = nr.assemble(A, R, D, cap, got["first_slot"], n, G, GAMMA, first, count)
            assert_assembled(got, ref)
            off = (got["first_slot"] - first) % cap
            assert (off < count).all()
            if count - (n - 1) * G > 0:
                assert (off < count - (n - 1) * G).all() and "incomplete" not in ref["cls"]
            if it >= 3:
                incomplete_late += ref["cls"].count("incomplete")
            if overlap:
                for _ in range(plies):
                    t.collect()
            t.learn_apply(1)
        assert incomplete_late == 0
        assert t.replay.stats()[2] > 2 * cap or plies == 1
        assert t.replay.stats()[2] > cap
    finally:
        t.close()


def test_overlapped_n_step_trainer_equals_its_sequential_definition(xq):
    """tests/test_trainer_gpu.py's composition with n_step = 3, 9 steps, bit for bit: the sequential definition draws from the same window
    cut by the newest 2 x 64 slots and lets the ring's default readable range stand (a superset that agrees on every chain it reads)"""
    import torch
    G, cap, mb, iters, n, sizes = 64, 64 * 5 + 21, 48, 9, 3, CFG2_NET
    seed, first_id = 99, 7
    cfg = xq.TrainerConfig(n_games=G, layer_sizes=sizes, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=cap,
                           minibatch=mb, td_net=1, backprop_mode=0, target_sync_interval=3, mean_gradient=1, seed=seed,
                           first_game_id=first_id, collects_per_update=1, overlap_collect=1)
    t = xq.Trainer(cfg)
    t.set_n_step(n)
    w0, b0 = t.dqn.get_params()
    t.step(iters)
    tw, tb = t.dqn.get_params()
    tboards, tmeta = t.env.get_state()
    tq = t.dqn.last_td_values(mb)
    env = xq.VecEnv(G, seed=seed, first_game_id=first_id)
    d = xq.DQN(sizes, 0.01, 0.99, seed=1)
    d.set_params(w0, b0); d.updateTargetNetwork()
    rp = xq.ReplayBuffer(cap, seed=seed + 0x1234567 + first_id)
    rp.set_n_step(n, G)

    def collect():
        q = d.q_boards(env, 96)
        env.selfplay_step_dev(q.data_ptr(), 96, 0.2, replay=rp)
        torch.cuda.synchronize()

    try:
        for it in range(iters):
            size, _, total = rp.stats()
            start, count = overlap_window(size, total, cap, G)
            if count <= 0:
                collect()
                size, _, total = rp.stats()
                start, count = default_range(size, total, cap)
                played = True
            else:
                played = False
            cut = count - (n - 1) * G if count - (n - 1) * G > 0 else count
            rp.sample_window(mb, start, cut)
            d.td_grads_replay(rp, mb, td_net=1, mode=0)
            if not played:
                collect()
            d.apply_grads(0.01, 1.0 / mb)
            if (it + 1) % 3 == 0:
                d.updateTargetNetwork()
        w, b = d.get_params()
        boards, meta = env.get_state()
        assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
        assert np.array_equal(w, tw) and np.array_equal(b, tb) and np.abs(w - w0).max() > 0
        q = d.last_td_values(mb)
        assert np.array_equal(q[0], tq[0]) and np.array_equal(q[1], tq[1])
    finally:
        t.close(); env.close(); d.close(); rp.close()


@pytest.mark.parametrize("warm", [0, 4])
def test_prioritized_trainer_holds_the_incomplete_chains(xq, warm):
    """prioritized replay with n_step = 3: once the ring holds 3 collects no drawn row is dead for an incomplete chain, and the batch is
    the reference over the range that goes with the tree (the filled ring minus the slots retired at the last learn_apply).  warm: plain
    iterations first — set_n_step then holds the newest slots out of the tree that is already there"""
    G, cap, mb, n, iters = 64, 64 * 6 + 19, 96, 3, 12
    cfg = xq.TrainerConfig(n_games=G, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.3, replay_capacity=cap,
                           minibatch=mb, td_net=2, target_sync_interval=3, seed=23, prioritized=1)
    t = xq.Trainer(cfg)
    try:
        rng_first, rng_count = None, None
        for _ in range(warm):
            t.collect(); t.learn_grads(); t.learn_apply(1)
            with pytest.raises(xq.XqError):
                t.dqn.last_n_step(1)
        if warm:
            size, _, total = t.replay.stats()
            rng_first, rng_count = tree_range(size, total, cap, G)
        t.set_n_step(n)
        late = 0
        for it in range(iters):
            t.collect()
            if rng_first is None:                                     # the first tree is built by learn_grads, from the ring as it stands
                size, _, total = t.replay.stats()
                rng_first, rng_count = default_range(size, total, cap)
            t.learn_grads()
            got = t.dqn.last_n_step(mb)
            A, R, D = ring_arrays(t.replay, cap)
            ref = nr.assemble(A, R, D, cap, got["first_slot"], n, G, GAMMA, rng_first, rng_count)
            assert_assembled(got, ref)
            if rng_count >= n * G:
                late += 1
                assert "incomplete" not in ref["cls"]
                assert ((got["first_slot"] - rng_first) % cap < rng_count - (n - 1) * G).all()
            t.learn_apply(1)
            size, _, total = t.replay.stats()
            rng_first, rng_count = tree_range(size, total, cap, G)
        assert late >= iters - 3 + min(warm, 3) and t.replay.stats()[2] > cap
    finally:
        t.close()


# ---- 6. refusals, and what the setting survives -------------------------------------------------------------------------------------
def test_refusals(xq, small):
    rp = xq.ReplayBuffer(40, seed=1)
    try:
        for bad in ((0, 1), (9, 1), (-1, 1), (2, 0), (2, 41), (3, 20), (8, 6), (2, 40)):
            with pytest.raises(xq.XqError) as e:
                rp.set_n_step(*bad)
            assert e.value.code == 1, bad
        assert rp.n_step == (1, 1)
        rp.set_n_step(8, 5)                                           # 7 * 5 = 35 < 40
        rp.set_n_step(2, 39)
        rp.enable_per(*PER)
        for bad in ((0, 0, -1, 0), (0, 0, 40, 0), (0, 0, 0, 41), (0, 0, 0, -1), (0, 41, 0, 0), (40, 0, 0, 0)):
            with pytest.raises(xq.XqError) as e:
                xq._capi.call("xq_replay_per_rebuild_hold", rp.handle, *bad)
            assert e.value.code == 1, bad
        plain = xq.ReplayBuffer(8, seed=1)
        with pytest.raises(xq.XqError):
            xq._capi.call("xq_replay_per_rebuild_hold", plain.handle, 0, 0, 0, 0)      # no priorities on this ring
        plain.close()
        fresh = xq.DQN(SMALL_NET, 0.01, 0.99, seed=1)
        with pytest.raises(xq.XqError) as e:
            fresh.last_n_step(1)
        assert e.value.code == 2
        fresh.close()
    finally:
        rp.close()
    fx = nr.named_fixture("partial37")
    rp = filled(xq, fx)
    try:
        rp.set_n_step(3, 4)
        rp.sample(8)
        small.td_grads_replay(rp, 8)
        small.apply_grads(0.0, 1.0)
        with pytest.raises(xq.XqError) as e:
            small.last_n_step(9)
        assert e.value.code == 1
        assert len(small.last_n_step(0)["reward"]) == 0
    finally:
        rp.close()
    mk = lambda **kw: xq.TrainerConfig(n_games=64, layer_sizes=SMALL_NET, minibatch=64, seed=1, **kw)
    for kw, n, code in ((dict(replay_capacity=0), 2, 1), (dict(replay_capacity=64 * 3), 3, 1), (dict(replay_capacity=64 * 3 + 1), 3, 0),
                        (dict(replay_capacity=64 * 4, collects_per_update=2), 3, 1), (dict(replay_capacity=64 * 4 + 1, collects_per_update=2), 3, 0),
                        (dict(replay_capacity=1024), 9, 1), (dict(replay_capacity=1024), 0, 1), (dict(replay_capacity=0), 1, 0)):
        t = xq.Trainer(mk(**kw))
        try:
            if code:
                with pytest.raises(xq.XqError) as e:
                    t.set_n_step(n)
                assert e.value.code == code, (kw, n)
                assert t.replay.n_step[0] == 1
            else:
                t.set_n_step(n)
                assert t.replay.n_step == (n, 64)
        finally:
            t.close()
    t = xq.Trainer(mk(replay_capacity=1024, overlap_collect=1))
    try:
        t.learn_grads()
        with pytest.raises(xq.XqError) as e:
            t.set_n_step(2)                                           # between iterations only
        assert e.value.code == 2
        t.collect(); t.learn_apply(1)
        t.set_n_step(2)
    finally:
        t.close()


def test_setting_survives_optimizer_params_and_model_load(xq, tmp_path):
    fx = nr.named_fixture("wrapped37")
    rp = filled(xq, fx)
    d, w, b = make_net(xq, SMALL_NET, seed=6, gamma=GAMMA)
    try:
        rp.set_n_step(3, 4)
        path = str(tmp_path / "m.bin")
        d.saveModel(path)
        for change in (lambda: d.set_optimizer("adam"), lambda: d.set_params(w, b), lambda: d.loadModel(path)):
            change()
            assert rp.n_step == (3, 4)
            slots = rp.sample(65)
            d.td_grads_replay(rp, 65)
            d.apply_grads(0.01, 1.0 / 65)
            assert_assembled(d.last_n_step(65), reference(fx, slots, 3))
    finally:
        d.close(); rp.close()


def test_facade_carries_n_step_onto_the_trainers_ring(xq):
    from test_nstep_ref_cpu import build_nstep_facade_probe
    exe = build_nstep_facade_probe()
    out = subprocess.run([exe, "64", "40", "7", "3"], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["ring_before"], r["ring_after"]) == (1, 3)
    assert r["nine_refused"] == 1 and r["long_refused"] == 1 and r["ai_nine_refused"] == 1
    assert r["plain_n"] == 1 and r["stepped_n"] == 3
    assert r["plain_updates"] > 0 and r["stepped_updates"] > 0
